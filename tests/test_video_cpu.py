"""CPU-side checks of the video writer (no GPU): the tables of audio2photoreal_amd/video.py and of tests/jpeg_restatement.py against
what Pillow itself writes (tests/golden/golden_video_v1.npz), the restatement's encoder against its decoder and against Pillow,
the AVI container of both, and the C ABI's names."""
import io
import os
import re
import struct

import numpy as np
import pytest
import torch

import jpeg_restatement as J
from audio2photoreal_amd import _lib
from audio2photoreal_amd import video as V
from audio2photoreal_amd._lib import A2PError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES, SUBS = (50, 90, 100), ("420", "444")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_video_v1.npz"))


@pytest.fixture(scope="module")
def images():
    return J.source_images()


@pytest.fixture(scope="module")
def files(images):
    return {(q, s): [J.encode(img, q, s) for img in images] for q in QUALITIES for s in SUBS}


# ------------------------------------------------------------------------------------------------ tables
def test_tables_and_huffman_specs_are_what_pillow_writes(gold):
    assert list(V.ZIGZAG) == J.ZIGZAG and sorted(J.ZIGZAG) == list(range(64))
    for q in QUALITIES:
        assert np.array_equal(V.quant_tables(q)[:, list(V.ZIGZAG)], gold[f"dqt/{q}"]), q
        assert np.array_equal(J.quant_tables(q).reshape(2, 64)[:, J.ZIGZAG], gold[f"dqt/{q}"]), q
    assert V.quant_tables(1).max() == 255 and V.quant_tables(100).max() == 1 and V.quant_tables(90).dtype == np.uint16
    for name in ("dc_luma", "ac_luma", "dc_chroma", "ac_chroma"):
        for spec in (V.HUFFMAN_SPECS[name], J.SPECS[name]):
            assert list(spec[0]) == list(gold[f"dht/{name}/bits"]) and list(spec[1]) == list(gold[f"dht/{name}/vals"]), name
    with pytest.raises(ValueError):
        V.quant_tables(0)
    with pytest.raises(ValueError):
        V.quant_tables(101)


def test_huffman_words_hold_the_codes_of_the_specs():
    words = V.huffman_words()
    assert words.shape == (_lib.JPEG_HUFF_WORDS,) and words.dtype == np.uint32
    seen = 0
    for base, name in ((0, "dc_luma"), (16, "dc_chroma"), (32, "ac_luma"), (288, "ac_chroma")):
        codes = J.huffman_codes(*J.SPECS[name])
        for sym, (code, length) in codes.items():
            assert words[base + sym] == (length << 16 | code)
        seen += len(codes)
        lengths = sorted(l for _, l in codes.values())
        assert sum(2.0 ** -l for l in lengths) < 1 and max(lengths) <= 16            # a prefix code with the all-ones word left free
    assert np.count_nonzero(words) == seen == 12 + 12 + 162 + 162
    # the capacity the kernel reserves per block: the longest DC symbol plus 63 times the longest AC symbol
    worst = max(l + s for n in ("dc_luma", "dc_chroma") for s, (_, l) in J.huffman_codes(*J.SPECS[n]).items())
    worst += 63 * max(l + (s & 15) for n in ("ac_luma", "ac_chroma") for s, (_, l) in J.huffman_codes(*J.SPECS[n]).items())
    assert worst == 1660 <= _lib.JPEG_BLOCK_BITS


def test_frame_header_is_the_restatement_s_and_in_the_issue_s_order():
    for (h, w), q, s in (((40, 72), 90, "420"), ((17, 33), 50, "444"), ((667, 2048), 100, "420")):
        head = V.frame_header(h, w, q, s)
        assert head == J.header(h, w, q, s)
        parsed = J.parse(head + b"\xff\xd9")
        assert parsed["order"] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA, 0xD9]
        assert parsed["size"] == (h, w) and parsed["dri"] == V.mcu_grid(h, w, s)[1]
    with pytest.raises(ValueError):
        V.frame_header(40, 72, 90, "422")
    with pytest.raises(ValueError):
        V.frame_header(0, 72)
    assert V.mcu_grid(40, 72, "420") == (3, 5, 6) and V.mcu_grid(40, 72, "444") == (5, 9, 3) and V.mcu_grid(17, 33, "420") == (2, 3, 6)


# ------------------------------------------------------------------------------------------------ the restatement against itself
def test_restatement_decoder_inverts_the_encoder_exactly(images, files):
    for (q, s), per_image in files.items():
        for img, data in zip(images, per_image):
            head, coef = J.decode_coefficients(data)
            assert np.array_equal(coef, J.coefficients(img, q, s)), (q, s)
            assert head["size"] == img.shape[:2]


def test_restatement_entropy_coder_on_edge_blocks():
    """A block without EOB, ZRL runs, the worst-case block and a DC swing survive the round trip through the bytes."""
    rng = np.random.default_rng(5)
    coef = np.zeros((2, 3, 6, 64), np.int16)
    coef[0, 0, 0, 63] = 5
    coef[0, 0, 1, 17], coef[0, 0, 2, 33], coef[0, 0, 3, 49] = -3, 1023, -1023
    coef[0, 1, 0, 0], coef[0, 1, 1, 0], coef[0, 1, 4, 0], coef[0, 2, 4, 0] = 1023, -1024, -1024, 1023
    coef[1, 0, 0] = np.where(np.arange(64) % 2, 1023, -1023)
    coef[1, 0, 0, 0] = -1024
    coef[1, 1] = rng.integers(-40, 41, size=(6, 64)) * (rng.random((6, 64)) < 0.2)
    data = J.header(32, 48, 90, "420") + J.entropy_segment(coef) + b"\xff\xd9"
    assert np.array_equal(J.decode_coefficients(data)[1], coef)
    # by hand from Tables K.3 - K.6: four luminance blocks "00" (category 0) "1010" (EOB), two chrominance blocks "00" "00"
    assert J.entropy_segment(coef[:1, :1] * 0) == bytes([0b00101000, 0b10100010, 0b10001010, 0b00000000])


# ------------------------------------------------------------------------------------------------ the restatement against Pillow
def test_pillow_reads_the_restatement_s_files(gold, images, files):
    """Pillow decodes the 4:4:4 files to within `idct_diff` of the restatement's decoder (its integer IDCT and its integer colour
    tables: at most 1 each, 2 measured and stored); 4:2:0 differs by design (Pillow interpolates chroma, the restatement
    replicates it), so there only the PSNR is compared.  The PSNR of Pillow's decode of the restatement's files falls short of that
    of Pillow's own files by at most the stored gap (0.086 dB, at quality 50, 4:2:0, smooth) plus 0.05 dB."""
    Image = pytest.importorskip("PIL.Image")
    gap, worst_pixel, worst_short = float(gold["gap"]), 0, -np.inf
    assert gap < 0.1 and int(gold["idct_diff"]) <= 2
    for (q, s), per_image in files.items():
        for i, (img, data) in enumerate(zip(images, per_image)):
            pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            assert pil.shape == img.shape
            if s == "444":
                worst_pixel = max(worst_pixel, int(np.abs(pil.astype(int) - J.decode(data).astype(int)).max()))
            short = float(gold[f"pil/{q}_{s}/psnr"][i]) - J.psnr(pil, img)
            worst_short = max(worst_short, short)
            assert short <= gap + 0.05, (q, s, i, short)
    print("largest pixel difference", worst_pixel, "largest PSNR shortfall", worst_short)
    assert worst_pixel <= int(gold["idct_diff"])


# ------------------------------------------------------------------------------------------------ the container
def _audio(samples, channels, seed=3):
    a = np.random.default_rng(seed).uniform(-1.3, 1.3, size=(samples, channels))
    a[:4] = [[-2.0] * channels, [2.0] * channels, [1.0] * channels, [-1.0] * channels]
    return a


def test_pcm_conversion_clips_and_rounds():
    x = np.array([0.0, 1.0, -1.0, 1.5, -7.0, 0.5, -0.5, 1e-5, 3.0518e-5])
    want = np.array([0, 32767, -32767, 32767, -32767, 16384, -16384, 0, 1])
    for f in (V.pcm16, J.pcm16):
        got = f(x)
        assert got.dtype == np.dtype("<i2") and got.shape == (9, 1) and np.array_equal(got[:, 0], want)
    assert np.array_equal(V.pcm16(_audio(100, 2)), J.pcm16(_audio(100, 2)))
    assert V.pcm16(torch.tensor([0.25, -0.25])).tolist() == [[8192], [-8192]]
    with pytest.raises(A2PError):
        V.pcm16(np.zeros((3, 2, 2)))
    with pytest.raises(A2PError):
        V.pcm16(np.zeros(5, np.int32))
    stored = np.array([[-32768, 32767], [5, -5]], np.int16)
    assert np.array_equal(V.pcm16(stored), stored)                              # PCM already: taken as it is


def _check_container(blob, frames, pcm, fps, size, rate):
    d = J.avi_demux(blob)
    assert d["riff_size"] + 8 == len(blob)
    assert d["frames"] == [bytes(f) for f in frames] and d["fps"] == pytest.approx(fps) and d["size"] == size
    assert d["video_length"] == len(frames) and d["avih"][4] == len(frames) and d["avih"][8:10] == (size[1], size[0])
    movi, movi_size = d["movi"]
    last = d["chunks"][-1]
    assert movi + movi_size == last[1] + 8 + last[2] + last[2] % 2                 # the list ends where its last chunk (padded) ends
    assert len(d["index"]) == len(d["chunks"])
    for (fourcc, flags, offset, size_), (cc, at, n) in zip(d["index"], d["chunks"]):
        assert (fourcc, movi + offset, size_) == (cc, at, n) and flags == 0x10
        assert blob[at:at + 4] == cc and struct.unpack_from("<I", blob, at + 4)[0] == n
        assert at % 2 == 0                                                       # every chunk starts on an even offset
    if pcm is None:
        assert d["audio"] is None and d["streams"] == [b"vids"] and d["avih"][6] == 1
    else:
        assert np.array_equal(d["audio"], pcm) and d["audio_rate"] == rate and d["audio_length"] == len(pcm) and d["avih"][6] == 2
    return d


def test_avi_mux_demux_round_trip(files):
    frames = files[90, "420"] + files[50, "444"] + [b"\xff\xd8\xff\xd9\x00"]        # an odd-sized chunk among them
    assert any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames)
    for fps, rate, channels, samples in ((30, 48000, 1, 7001), (30, 48000, 2, 3), (2, 44101, 2, 44101 * 4 + 17), (29.97, 16000, 1, 0), (3, None, 0, 0)):
        pcm = None if rate is None else J.pcm16(_audio(max(samples, 4), channels))[:samples]
        blob = J.avi_mux(frames, 40, 72, fps, pcm, rate)
        d = _check_container(blob, frames, pcm, fps, (40, 72), rate)
        kinds = [c[0] for c in d["chunks"]]
        if rate == 44101:            # 7 frames at 2 fps: audio of a second in front of its frames, the rest behind the last frame
            assert kinds == [b"01wb", b"00dc", b"00dc", b"01wb", b"00dc", b"00dc", b"01wb", b"00dc", b"00dc", b"01wb", b"00dc", b"01wb"]
            assert [c[2] for c in d["chunks"] if c[0] == b"01wb"] == [44101 * 4] * 4 + [17 * 4]
        got = V.read_video(_tmp(blob))
        assert got["frames"] == [bytes(f) for f in frames] and got["fps"] == pytest.approx(fps) and got["size"] == (40, 72)
        if pcm is None:
            assert got["audio"] is None and got["audio_rate"] is None
        else:
            assert np.array_equal(got["audio"], pcm[:, 0] if channels == 1 else pcm) and got["audio_rate"] == rate


def _tmp(blob, _dir=[]):
    import tempfile
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix="a2p_video_"))
    path = os.path.join(_dir[0], "clip.avi")
    open(path, "wb").write(blob)
    return path


def test_writer_container_equals_the_restatement_s_with_the_encoder_stubbed(files, tmp_path, monkeypatch):
    """MJPEGWriter's file, byte for byte, with canned JPEG files in place of the GPU encoder: several write() calls, audio in mono
    and stereo at a rate 30 does not divide, and the size guard."""
    canned = files[90, "420"] + files[100, "444"] + files[50, "420"] + [b"\xff\xd8\xff\xd9\x00"]

    def fake_encode(frames, quality=90, subsampling="420", max_bytes=0):
        picked = [canned[int(i)] for i in frames[:, 0, 0, 0]]
        off = np.concatenate([[0], np.cumsum([len(p) for p in picked])]).astype(np.int64)
        return np.frombuffer(b"".join(picked), np.uint8), off

    monkeypatch.setattr(V, "encode_jpeg_frames", fake_encode)
    monkeypatch.setattr(V, "_frames_arg", lambda f: f)
    ids = torch.arange(len(canned), dtype=torch.uint8).reshape(-1, 1, 1, 1).expand(-1, 40, 72, 3)
    for fps, rate, channels, samples, cuts in ((30, 48000, 2, 9000, (0, 10)), (3, 44101, 1, 44101 * 5, (0, 1, 4, 7, 10)), (2.5, 8000, 2, 100, (0, 10)),
                                               (4, None, 0, 0, (0, 5, 10))):
        audio = None if rate is None else _audio(samples, channels)
        path = tmp_path / f"clip_{fps}.avi"
        with V.MJPEGWriter(path, 40, 72, fps=fps, audio=audio, audio_rate=rate) as w:
            for a, b in zip(cuts[:-1], cuts[1:]):
                assert w.write(ids[a:b]) == b
        blob = open(path, "rb").read()
        pcm = None if rate is None else J.pcm16(audio)
        assert blob == J.avi_mux(canned, 40, 72, fps, pcm, rate)
        _check_container(blob, canned, pcm, fps, (40, 72), rate)
    # the size guard: nothing of the refused call is written, and close() finalises what is there
    audio = _audio(48000, 1)
    one = len(J.avi_mux(canned[:3], 40, 72, 30, J.pcm16(audio), 48000))
    monkeypatch.setattr(V, "AVI_LIMIT", one + 100)
    path = tmp_path / "guard.avi"
    w = V.MJPEGWriter(path, 40, 72, fps=30, audio=audio, audio_rate=48000)
    w.write(ids[:3])
    with pytest.raises(ValueError, match="2 GiB"):
        w.write(ids[3:6])
    w.close()
    blob = open(path, "rb").read()
    assert len(blob) == one <= V.AVI_LIMIT and blob == J.avi_mux(canned[:3], 40, 72, 30, J.pcm16(audio), 48000)
    with pytest.raises(ValueError, match="closed"):
        w.write(ids[:1])
    with pytest.raises(A2PError):
        V.MJPEGWriter(tmp_path / "x.avi", 40, 72).write(ids[:1, :8])           # another frame size
    with pytest.raises(ValueError):
        V.MJPEGWriter(tmp_path / "y.avi", 40, 72, audio=audio)                  # audio without a rate


def test_frames_must_be_uint8_on_the_gpu():
    with pytest.raises(A2PError, match="MI355X"):
        V.encode_jpeg_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(A2PError, match="torch tensor"):
        V.coefficients(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(A2PError, match="MI355X"):
        V.entropy_segments(torch.zeros(1, 1, 1, 3, 64, dtype=torch.int16))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_names_and_constants():
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    for name in ("a2p_jpeg_coefficients", "a2p_jpeg_entropy"):
        assert name in _lib.EXPORTS and re.search(rf"\bint {name}\(", header)
    for name, value in (("A2P_JPEG_MAX_SIZE", _lib.JPEG_MAX_SIZE), ("A2P_JPEG_BLOCK_BITS", _lib.JPEG_BLOCK_BITS),
                        ("A2P_JPEG_HUFF_WORDS", _lib.JPEG_HUFF_WORDS)):
        assert re.search(rf"#define {name} (\d+)", header).group(1) == str(value)
    kernels = open(os.path.join(ROOT, "audio2photoreal_amd", "csrc", "kernels_video.h")).read()
    assert re.search(r"#define JPEG_BLOCK_BITS (\d+)", kernels).group(1) == str(_lib.JPEG_BLOCK_BITS)
    assert [int(x) for x in re.search(r"JPEG_ZIGZAG_POS\[64\] = \{([^}]*)\}", kernels).group(1).split(",")] == list(np.argsort(J.ZIGZAG))
