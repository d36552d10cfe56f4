"""The JPEG reader on the MI355X (audio2photoreal_amd/video.py decode_jpeg_frames, MJPEGReader; csrc/kernels_video_decode.h) against
the numpy restatements: entropy decoding is lossless and is compared element for element; pixels are compared with the float64
decode under the rule of jpeg_decode_restatement.check_pixels: equal, except where the float64 value before rounding lies within
1e-3 of a half-integer (ten times what a numpy fp32 run of the same arithmetic deviates), where it may differ by 1."""
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpeg_decode_restatement as D
import jpeg_restatement as J
from audio2photoreal_amd import video as V
from audio2photoreal_amd._lib import A2PError
from conftest import record
from test_video_hip import crafted

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
BAND_SHARE = 0.01                   # the share of pixels the rule may excuse; the float64 reference alone gives about 0.2 %


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def images():
    return J.source_images()


@functools.lru_cache(maxsize=None)
def encoded(n, q, s):
    """(file, its coefficients by jpeg_restatement.decode_coefficients, float64 pixels before rounding) of source image n."""
    data = J.encode(J.source_images()[n], q, s)
    h, coef = J.decode_coefficients(data)
    h["sampling"] = s
    return data, coef, D.pixels64(h, coef)


def check_frames(got, exacts, name=None):
    """got uint8 [N, H, W, 3] (a tensor) under the pixel rule against the float64 values; records and bounds the excused share."""
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(exacts),) + exacts[0].shape
    shares, wrong, worst = [], 0, 0.0
    for g, e in zip(got, exacts):
        share, bad = D.check_pixels(g, e)
        shares.append(share)
        wrong += bad
        miss = g.astype(np.int64) != np.clip(np.rint(e), 0, 255)
        if miss.any():                                              # a pixel that rounds the other way: the GPU value was at least this far off
            worst = max(worst, float(np.abs(e - np.floor(e) - 0.5)[miss].max()))
    if name:
        record(name, band_share=max(shares), differing_pixels=wrong, gpu_deviation_at_least=worst)
    return max(shares), wrong


# ------------------------------------------------------------------------------------------------ 1. entropy decoding
@pytest.mark.parametrize("s", ("420", "444"))
@pytest.mark.parametrize("q", (10, 50, 90, 100))
def test_entropy_decoding_is_exact_on_the_source_images(dev, q, s):
    files = [encoded(n, q, s) for n in range(3)]
    coef, h = V.decode_coefficients([f[0] for f in files])
    assert coef.dtype == torch.int16 and tuple(coef.shape) == (3, *V.mcu_grid(40, 72, s), 64) and h["sampling"] == s
    got = coef.cpu().numpy()
    for n in range(3):
        assert np.array_equal(got[n], files[n][1]), (q, s, n)
    data = np.frombuffer(b"".join(f[0] for f in files), np.uint8)
    off = np.cumsum([0] + [len(f[0]) for f in files])
    assert torch.equal(V.decode_coefficients(data, off)[0], coef)                  # one array with offsets is the same input


@pytest.mark.parametrize("kind", ("worst", "runs", "only63", "dcswing", "alternating", "zero"))
def test_entropy_decoding_is_exact_on_crafted_blocks(dev, kind):
    """The 1660-bit block, ZRL runs, a non-zero coefficient 63 without EOB, DC differences of +-2047."""
    rng = np.random.default_rng(17)
    for s, bpm in (("420", 6), ("444", 3)):
        coef = crafted(kind, (2, 2, 3, bpm, 64), rng)
        mcu = 16 if bpm == 6 else 8
        files = [D.encode_coefficients(c, 2 * mcu, 3 * mcu, 90, s, 3) for c in coef]
        for f, c in zip(files, coef):
            assert np.array_equal(J.decode_coefficients(f)[1], c)
        got, _ = V.decode_coefficients(files)
        assert np.array_equal(got.cpu().numpy(), coef), (kind, s)


# ------------------------------------------------------------------------------------------------ 2. the GPU's own round trip
@pytest.mark.parametrize("bpm", (6, 3))
@pytest.mark.parametrize("grid", ((1, 1), (1, 17), (9, 5), (3, 70)), ids=("1x1", "1x17", "9x5", "3x70"))
def test_gpu_round_trip_of_random_coefficients(dev, grid, bpm):
    """decode_coefficients(entropy_segments(coef)) is coef.  9 rows: RST7 is followed by RST0; 70 columns: more than the 64 blocks of
    one chunk of the encoder; three frames of different density, so of different length; one frame made to hold runs of 0xFF bytes."""
    rows, cols = grid
    rng = np.random.default_rng(1000 * rows + cols + bpm)
    shape = (3, rows, cols, bpm, 64)
    coef = rng.integers(-1023, 1024, size=shape) * (rng.random(shape) < np.array([0.05, 0.5, 1.0]).reshape(3, 1, 1, 1, 1))
    coef[..., 0] = rng.integers(-1024, 1024, size=shape[:-1])
    coef = coef.astype(np.int16)
    coef[2] = crafted("stuffing", (1,) + shape[1:], rng)[0]
    s, mcu = ("420", 16) if bpm == 6 else ("444", 8)
    t = torch.from_numpy(coef).to(dev)
    stream, off = V.entropy_segments(t, head=V.frame_header(rows * mcu, cols * mcu, 90, s), tail=V.EOI)
    raw = stream.cpu().numpy()
    assert len(set(np.diff(off))) == 3 and raw[off[2]:].tobytes().count(b"\xff\x00") >= 20
    got, h = V.decode_coefficients(raw, off)
    assert h["dri"] == cols and torch.equal(got, t)
    alone, _ = V.decode_coefficients(raw[off[1]:off[2]].tobytes())
    assert torch.equal(alone[0], t[1])


# ------------------------------------------------------------------------------------------------ 3. layouts the encoder never writes
LAYOUT_CASES = [(s, ri, custom, dht) for s in ("420", "422", "444", "gray")
                for ri, custom, dht in ((0, False, True), (1, False, True), (3, True, True), ("cols", False, False), (999, True, True))]


@pytest.mark.parametrize("s", ("420", "422", "444", "gray"))
def test_layouts_the_encoder_never_writes(dev, images, s):
    """Ri in {0, 1, 3, mcu_cols, more than all MCUs}, Huffman tables that are not Annex K (every one with a 16-bit code), no DHT, for
    every sampling: exact coefficients, pixels by the rule."""
    img = images[2][:23, :37]
    cols = D.grid(23, 37, s)[1]
    coef = D.coefficients(img, 75, s)
    files = [D.encode_coefficients(coef, 23, 37, 75, s, cols if ri == "cols" else ri, D.custom_specs() if custom else J.SPECS, dht)
             for _, ri, custom, dht in (c for c in LAYOUT_CASES if c[0] == s)]
    h, want = D.decode_coefficients(files[0])
    assert np.array_equal(want, coef)
    exact = D.pixels64(h, want)
    for f in files:
        got, hdr = V.decode_coefficients(f)
        assert np.array_equal(got.cpu().numpy()[0], coef) and hdr["sampling"] == s
    frames = V.decode_jpeg_frames(files)                                           # five headers: five groups of one frame
    share, _ = check_frames(frames, [exact] * len(files), f"video_decode_layout_{s}")
    assert share <= BAND_SHARE
    assert all(torch.equal(frames[0], f) for f in frames[1:])                      # the same coefficients and tables: the same bytes


def test_pil_files_decode_to_the_restatement_s_pixels(dev, images):
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(images[2])
    cases = {"444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2), "420_optimize": dict(subsampling=2, optimize=True),
             "420_rst_rows": dict(subsampling=2, restart_marker_rows=1), "444_rst_blocks": dict(subsampling=0, restart_marker_blocks=3),
             "gray": None}
    figures = {}
    for name, kw in cases.items():
        f = io.BytesIO()
        (img.convert("L") if kw is None else img).save(f, "JPEG", quality=85, **(kw or {}))
        data = f.getvalue()
        h, coef = D.decode_coefficients(data)
        got, _ = V.decode_coefficients(data)
        assert np.array_equal(got.cpu().numpy()[0], coef), name
        frames = V.decode_jpeg_frames([data])
        share, _ = check_frames(frames, [D.pixels64(h, coef)])
        assert share <= BAND_SHARE
        pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.int64)
        figures[name] = int(np.abs(frames[0].cpu().numpy().astype(np.int64) - pil).max())
    record("video_decode_vs_pil_max_abs", **figures)
    # libjpeg's integer IDCT against float64: at most 2 levels without upsampling; with it the two differ by design (replication
    # here, the triangle filter there), and only the figure is written down
    assert figures["444"] <= 2 and figures["444_rst_blocks"] <= 2 and figures["gray"] <= 2, figures


# ------------------------------------------------------------------------------------------------ 4. pixels against float64
def overshoot_file(height, width, s, seed):
    """A file whose IDCT leaves [0, 255] on both sides in every block: large random coefficients under the quality-50 tables."""
    rng = np.random.default_rng(seed)
    coef = rng.integers(-40, 41, size=D.grid(height, width, s) + (64,)) * (rng.random(64) < 0.3)
    coef[..., 0] = rng.integers(-20, 21, size=coef.shape[:-1])
    return D.encode_coefficients(coef.astype(np.int16), height, width, 50, s, 2)


@pytest.mark.parametrize("size", ((1, 1), (7, 9), (17, 33), (40, 72)), ids=("1x1", "7x9", "17x33", "40x72"))
def test_pixels_equal_float64_outside_the_band(dev, images, size):
    H, W = size
    files, exacts = [], []
    for s in ("420", "444", "422", "gray"):
        for q in (50, 95):
            files.append(D.encode(images[2][:H, :W], q, s))
        files.append(overshoot_file(H, W, s, H + W))
    for f in files:
        exacts.append(D.pixels64(*D.decode_coefficients(f)))
    h, coef = D.decode_coefficients(files[2])                                      # the overshoot is there: both clamps of A.3.1 work
    nat = np.zeros(coef.shape)
    nat[..., J.ZIGZAG] = coef * np.stack([h["dqt"][t] for t in (0, 0, 0, 0, 1, 1)])
    C = J.dct_matrix()
    raw = np.einsum("vy,rckvu,ux->rckyx", C, nat.reshape(coef.shape[:3] + (8, 8)), C) + 128
    assert raw.min() < -50 and raw.max() > 305
    frames = V.decode_jpeg_frames(files)
    share, _ = check_frames(frames, exacts, f"video_decode_pixels_{H}x{W}")
    assert share <= BAND_SHARE, share
    if size == (40, 72):                                                           # the two stages by hand give the same bytes
        data, want, exact = encoded(1, 90, "420")
        coef_t, hdr = V.decode_coefficients(data)
        px = V.pixels(coef_t, 40, 72, V.header_qtabs(hdr), "420")
        assert torch.equal(px, V.decode_jpeg_frames([data]))
        assert check_frames(px, [exact])[0] <= BAND_SHARE


# ------------------------------------------------------------------------------------------------ 5. strides, N, slicing
@pytest.mark.parametrize("s", ("420", "444"))
def test_decoding_into_a_window_and_independence_of_n(dev, s):
    files = [encoded(n, 90, s)[0] for n in range(3)]
    dense = V.decode_jpeg_frames(files)
    wide = torch.full((3, 40 + 2, 3 * 72 + 5, 3), CANARY, dtype=torch.uint8, device=dev)
    for x0 in (0, 72 + 1, 2 * 72 + 5):                                             # byte offsets that are and are not multiples of 4
        wide.fill_(CANARY)
        window = wide[:, 1:41, x0:x0 + 72]
        assert V.decode_jpeg_frames(files, out=window) is window
        assert torch.equal(window, dense)
        keep = torch.ones_like(wide, dtype=torch.bool)
        keep[:, 1:41, x0:x0 + 72] = False
        assert bool((wide[keep] == CANARY).all())
    for n in range(3):                                                             # a frame's bytes: not its index, N or the slicing
        assert torch.equal(V.decode_jpeg_frames([files[n]])[0], dense[n])
    assert torch.equal(V.decode_jpeg_frames(files[::-1]), dense.flip(0))
    assert torch.equal(V.decode_jpeg_frames(files, max_bytes=1), dense)
    mixed = [files[0], encoded(0, 50, s)[0], files[1], encoded(1, 50, s)[0]]         # two headers interleaved: groups, frames in place
    got = V.decode_jpeg_frames(mixed)
    assert torch.equal(got[0], dense[0]) and torch.equal(got[2], dense[1])
    assert torch.equal(got[1], V.decode_jpeg_frames([mixed[1]])[0])
    with pytest.raises(A2PError, match="out must"):
        V.decode_jpeg_frames(files, out=wide[:, 1:41, :72].permute(0, 2, 1, 3))
    with pytest.raises(A2PError, match="share one size"):
        V.decode_jpeg_frames([files[0], J.encode(J.source_images(24, 40)[0], 90, s)])


# ------------------------------------------------------------------------------------------------ 6. rejected input
def test_bad_frames_are_rejected_by_design_and_their_neighbours_decode(dev, images):
    """The streams of jpeg_decode_restatement.bad_streams, which tests/test_video_decode_cpu.py first runs through the host program
    under sanitizers: each is refused with its frame, interval and cause; the other frames of the batch decode exactly; the guard
    bytes around the output keep their fill."""
    good = [encoded(n, 90, "420") for n in range(3)]
    bad = D.bad_streams(J.coefficients(images[0], 90, "420"), 40, 72)
    assert sorted(bad) == ["ends_in_code", "no_code", "rst_order", "run_past_63", "truncated"]
    from audio2photoreal_amd import _lib
    for name, (data, interval, cause) in bad.items():
        batch = [good[0][0], data, good[1][0], good[2][0]]
        text = f"frame 1 is rejected: interval {interval}: {_lib.JPEG_CAUSES[cause]}"
        with pytest.raises(A2PError) as e:
            V.decode_jpeg_frames(batch)
        assert text in str(e.value), (name, str(e.value))
        with pytest.raises(A2PError) as e:
            V.decode_coefficients([data])
        assert f"frame 0 is rejected: interval {interval}: {_lib.JPEG_CAUSES[cause]}" in str(e.value), (name, str(e.value))
        guard = torch.full((6, 40, 72, 3), CANARY, dtype=torch.uint8, device=dev)
        frames, marked = V.decode_jpeg_frames(batch, out=guard[1:5], on_error="mark")
        assert marked == [1], name
        assert bool((guard[0] == CANARY).all()) and bool((guard[5] == CANARY).all()) and bool((frames[1] == 0).all())
        for k, n in ((0, 0), (2, 1), (3, 2)):
            assert check_frames(frames[k:k + 1], [good[n][2]])[1] >= 0
            assert torch.equal(frames[k], V.decode_jpeg_frames([good[n][0]])[0]), (name, k)


# ------------------------------------------------------------------------------------------------ 7. files
def test_files_read_back_as_the_frames_of_their_jfif_strings(dev, images, tmp_path):
    rng = np.random.default_rng(9)
    frames = np.concatenate([images, images[::-1], images[:1]])                    # 7 frames
    audio = rng.uniform(-1, 1, size=(2 * 8000 + 123, 2))
    path = tmp_path / "clip.avi"
    assert V.write_video(path, torch.from_numpy(frames).to(dev), fps=3, quality=90, audio=audio, audio_rate=8000, slice_frames=4) == 7
    jfif = V.read_video(path)["frames"]
    want = V.decode_jpeg_frames(jfif)
    with V.MJPEGReader(path, slice_frames=3) as r:
        assert len(r) == 7 and r.fps == 3 and r.size == (40, 72) and r.audio_rate == 8000
        assert [r.frame_bytes(i) for i in range(7)] == jfif
        assert np.array_equal(r.audio, V.pcm16(audio))
        assert torch.equal(r.read(), want) and torch.equal(r.read(2, 3), want[2:5]) and r.read(7, 0).shape == (0, 40, 72, 3)
        slices = list(r)
        assert [len(s) for s in slices] == [3, 3, 1] and torch.equal(torch.cat(slices), want)
        with pytest.raises(A2PError, match="outside the file"):
            r.read(5, 3)
    for step in (2, 64):                                                           # two slice sizes: the same bits
        got = V.read_video_frames(path, slice_frames=step)
        assert torch.equal(got["frames"], want) and got["fps"] == 3 and got["audio_rate"] == 8000
        assert np.array_equal(got["audio"], V.pcm16(audio))
    assert torch.equal(V.read_video_frames(path, 1, 5, slice_frames=2)["frames"], want[1:6])
    mine = [J.psnr(a, b) for a, b in zip(want.cpu().numpy(), frames)]
    theirs = [J.psnr(D.decode(f), b) for f, b in zip(jfif, frames)]
    record("video_decode_round_trip_q90_420", psnr_gpu_decoder=[round(p, 3) for p in mine], psnr_restatement_decoder=[round(p, 3) for p in theirs])
    assert max(abs(a - b) for a, b in zip(mine, theirs)) < 0.01                    # the pixels agree by the rule, so the PSNRs do
    share, _ = check_frames(want, [D.pixels64(*D.decode_coefficients(f)) for f in jfif])
    assert share <= BAND_SHARE


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_command_line_extracts_the_frames_pngs_and_audio(dev, images, tmp_path):
    import wave
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(4)
    audio = rng.uniform(-1, 1, size=9000)
    path = tmp_path / "clip.avi"
    V.write_video(path, torch.from_numpy(np.concatenate([images, images])).to(dev), fps=30, audio=audio, audio_rate=8000)
    want = V.read_video_frames(path)["frames"].cpu().numpy()
    out, pngs, wav = tmp_path / "frames.npy", tmp_path / "png", tmp_path / "a.wav"
    r = subprocess.run([sys.executable, "-m", "audio2photoreal_amd.video", "--extract", str(path), "--out", str(out), "--frames", "1:5",
                        "--png-dir", str(pngs), "--wav", str(wav), "--slice-frames", "3"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frames 1 .. 4 of 6" in r.stdout and "4 png files" in r.stdout
    assert np.array_equal(np.load(out), want[1:5])
    assert sorted(os.listdir(pngs)) == [f"frame_00_{t:05d}.png" for t in range(1, 5)]
    for t in range(1, 5):
        assert np.array_equal(np.asarray(Image.open(pngs / f"frame_00_{t:05d}.png")), want[t])
    with wave.open(str(wav), "rb") as w:
        assert w.getframerate() == 8000 and w.getnchannels() == 1
        assert np.array_equal(np.frombuffer(w.readframes(w.getnframes()), "<i2"), V.pcm16(audio)[:, 0])
    assert V.main(["--extract", str(path), "--out", str(out)]) == 0 and np.array_equal(np.load(out), want)
