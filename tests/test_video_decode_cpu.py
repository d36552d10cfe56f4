"""CPU-side checks of the JPEG reader (audio2photoreal_amd/video.py): the generalised numpy restatement against the one it
generalises, the host header parser against both restatements and PIL, the rejections, the AVI index, the C ABI's declarations, and
the decoding core (csrc/jpeg_decode_core.h) compiled into a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer and run on valid and corrupted streams.  Nothing here needs a GPU."""
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_decode_restatement as D
import jpeg_restatement as J
from audio2photoreal_amd import _lib
from audio2photoreal_amd import video as V
from audio2photoreal_amd._lib import A2PError
from test_video_hip import crafted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def images():
    return J.source_images()


def same_header(got, want, data):
    """parse_jpeg_header's dict against a restatement's parse of the same file."""
    assert got["size"] == tuple(want["size"])
    assert got["components"] == want["components"] and got["scan"] == want["scan"] and got["dri"] == want["dri"]
    assert sorted(got["dqt"]) == sorted(want["dqt"])
    for k in want["dqt"]:
        assert got["dqt"][k].dtype == np.uint16 and np.array_equal(got["dqt"][k], want["dqt"][k])
    assert {k: (list(b), list(v)) for k, (b, v) in got["dht"].items()} == {k: (list(b), list(v)) for k, (b, v) in want["dht"].items()}
    a, b = got["segment"]
    assert bytes(data[a:b]) == want["segment"]
    assert got["order"] == want["order"]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("s", ("420", "444"))
def test_the_generalised_restatement_is_the_old_one_where_that_applies(images, s):
    for q in (10, 90):
        for img in images[:2]:
            data = J.encode(img, q, s)
            assert D.encode(img, q, s) == data
            h0, c0 = J.decode_coefficients(data)
            h1, c1 = D.decode_coefficients(data)
            assert np.array_equal(c0, c1) and h1["sampling"] == s
            assert np.array_equal(J.decode(data), D.decode(data))


@pytest.mark.parametrize("s", ("422", "gray", "420", "444"))
def test_the_generalised_restatement_round_trips_its_own_layouts(images, s):
    img = images[2][:23, :37]
    coef = D.coefficients(img, 75, s)
    rows, cols, bpm = D.grid(23, 37, s)
    assert coef.shape == (rows, cols, bpm, 64)
    for ri, specs, dht in ((0, J.SPECS, True), (1, J.SPECS, True), (3, D.custom_specs(), True), (cols, J.SPECS, False), (rows * cols + 5, J.SPECS, True)):
        data = D.encode_coefficients(coef, 23, 37, 75, s, ri, specs, dht)
        h, got = D.decode_coefficients(data)
        assert np.array_equal(got, coef), (s, ri)
        assert (0xC4 in h["order"]) == dht and h["dri"] == ri
    got = D.decode(data).astype(np.float64)
    ref = img.astype(np.float64) if s != "gray" else np.repeat(np.rint(0.299 * img[..., :1] + 0.587 * img[..., 1:2] + 0.114 * img[..., 2:]), 3, -1)
    assert J.psnr(got, ref) > 24, (s, J.psnr(got, ref))               # a sanity bound on the pixel path of the new layouts
    assert max(len(J.huffman_codes(*t)) for t in D.custom_specs().values()) == 162
    assert all(max(l for _, l in J.huffman_codes(*t).values()) == 16 for t in D.custom_specs().values())


# ------------------------------------------------------------------------------------------------ the header parser
def test_parse_jpeg_header_equals_the_restatement_s(images):
    for s in ("420", "444"):
        data = J.encode(images[0], 90, s)
        got = V.parse_jpeg_header(data)
        same_header(got, J.parse(data), data)
        assert got["sampling"] == s and not got["default_dht"]
    for s, ri, specs, dht in (("422", 3, D.custom_specs(), True), ("gray", 0, J.SPECS, True), ("420", 5, J.SPECS, False)):
        data = D.encode(images[1], 50, s, ri, specs, dht)
        got = V.parse_jpeg_header(np.frombuffer(data, np.uint8))
        same_header(got, D.parse(data), data)
        assert got["sampling"] == s and got["default_dht"] == (not dht)
        assert V.decode_grid(got) == D.grid(40, 72, s)
    assert V.header_qtabs(got).shape == (3, 64)


def test_parse_jpeg_header_on_pil_files(images):
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(images[2])
    cases = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, optimize=True),
             dict(subsampling=2, restart_marker_rows=1), dict(subsampling=0, restart_marker_blocks=3)]
    names = ["444", "422", "420", "420", "420", "444"]
    for kw, name in zip(cases, names):
        f = io.BytesIO()
        img.save(f, "JPEG", quality=85, **kw)
        data = f.getvalue()
        got = V.parse_jpeg_header(data)
        same_header(got, D.parse(data), data)
        assert got["sampling"] == name and not got["default_dht"]
    assert got["dri"] == 3
    f = io.BytesIO()
    img.convert("L").save(f, "JPEG", quality=85)
    got = V.parse_jpeg_header(f.getvalue())
    same_header(got, D.parse(f.getvalue()), f.getvalue())
    assert got["sampling"] == "gray"


def patched(data, marker, fn):
    """The file with the body of its first `marker` segment replaced by fn(body)."""
    at = data.index(bytes([0xFF, marker]))
    n = struct.unpack_from(">H", data, at + 2)[0]
    body = fn(bytearray(data[at + 4:at + 2 + n]))
    return data[:at + 2] + struct.pack(">H", len(body) + 2) + bytes(body) + data[at + 2 + n:]


def test_unsupported_formats_are_rejected_by_name(images):
    data = J.encode(images[0][:16, :16], 90, "420")

    def with_sof(code):
        at = data.index(b"\xff\xc0")
        return data[:at + 1] + bytes([code]) + data[at + 2:]

    def set_byte(i, v):
        def fn(b):
            b[i] = v
            return b
        return fn

    cases = [(with_sof(0xC2), "progressive"), (with_sof(0xC1), "extended"), (with_sof(0xC9), "arithmetic"),
             (patched(data, 0xC0, set_byte(0, 12)), "12-bit samples"),
             (patched(data, 0xDB, lambda b: bytearray([0x10]) + bytearray(128)), "16-bit quantisation tables"),
             (patched(data, 0xC0, lambda b: set_byte(5, 4)(b + bytearray([4, 0x11, 0]))), "4 components"),
             (patched(data, 0xC0, set_byte(7, 0x41)), "sampling factors"),
             (patched(data, 0xC0, set_byte(7, 0x12)), "sampling factors"),
             (patched(data, 0xC0, set_byte(10, 0x21)), "sampling factors"),
             (patched(data, 0xDA, lambda b: b[:-3] + bytearray([0, 5, 0])), "spectral selection"),
             (b"\x89PNG" + data, "SOI")]
    for bad, word in cases:
        with pytest.raises(A2PError, match=word):
            V.parse_jpeg_header(bad)
    with pytest.raises(A2PError, match="frame 1: .*progressive"):
        V._parse_all(*V._jpeg_files([data, with_sof(0xC2)], None))
    with pytest.raises(A2PError, match="sampling="):
        V.pixels(None, 8, 8, np.ones((3, 64)), "411")


def test_decoder_tables_follow_annex_c():
    for name, (bits, vals) in list(V.HUFFMAN_SPECS.items()) + list(D.custom_specs().items()):
        t = V.decoder_table(tuple(bits), tuple(vals))
        symbols = t[32:].view(np.uint8)
        for sym, (code, length) in J.huffman_codes(bits, vals).items():
            assert t[length - 1] >= code, name
            assert symbols[code + t[16 + length - 1]] == sym, name
        assert all(t[l] == -1 for l in range(16) if not bits[l])
    with pytest.raises(A2PError, match="prefix code"):
        V.decoder_table((3,) + (0,) * 15, (1, 2, 3))


# ------------------------------------------------------------------------------------------------ the container
def test_mjpeg_reader_indexes_the_chunks_avi_demux_finds(tmp_path):
    rng = np.random.default_rng(5)
    frames = [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (101, 64, 7, 300, 1)]      # odd sizes: padded chunks
    audio = rng.integers(-2000, 2000, size=(2 * 8000 + 333, 2)).astype("<i2")
    for name, kw in (("av.avi", dict(audio=audio, audio_rate=8000)), ("v.avi", {})):
        blob = J.avi_mux(frames, 24, 40, 2.5, **kw)
        path = tmp_path / name
        path.write_bytes(blob)
        want = J.avi_demux(blob)
        with V.MJPEGReader(path) as r:
            assert len(r) == 5 and r.fps == want["fps"] and r.size == want["size"] and r.audio_rate == want["audio_rate"]
            assert [r.frame_bytes(i) for i in range(5)] == want["frames"]
            assert r.chunks == [(a + 8, n) for fourcc, a, n in want["chunks"] if fourcc == b"00dc"]
            assert (r.audio is None) == (want["audio"] is None)
            if kw:
                assert np.array_equal(r.audio, want["audio"])
        old = V.read_video(path)
        assert old["frames"] == want["frames"]
    (tmp_path / "not.avi").write_bytes(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        V.MJPEGReader(tmp_path / "not.avi")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_new_exports_are_declared_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a2p_hip.h")).read(), flags=re.S)
    for name in ("a2p_jpeg_restarts", "a2p_jpeg_decode_entropy", "a2p_jpeg_pixels"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
    for macro, value in (("A2P_JPEG_TABLES", _lib.JPEG_TABLES), ("A2P_JPEG_TABLE_WORDS", _lib.JPEG_TABLE_WORDS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    causes = {int(v) for v in re.findall(r"#define A2P_JPEG_ERR_[A-Z_]+ (\d+)", src)}
    assert causes == set(_lib.JPEG_CAUSES)
    core = open(os.path.join(ROOT, "audio2photoreal_amd", "csrc", "jpeg_decode_core.h")).read()
    assert {int(v) for v in re.findall(r"#define JPEG_ERR_[A-Z_]+ (\d+)", core)} == causes


# ------------------------------------------------------------------------------------------------ the decoding core under sanitizers
# leak detection is off: it needs ptrace, which a sandbox may refuse, and the subject here is out-of-bounds access
SANITIZER_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def sanitizer_compiler(tmp):
    """A C++ compiler that links AddressSanitizer and UndefinedBehaviorSanitizer programs that run, or None."""
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            exe = tmp / "probe"
            r = subprocess.run([cxx, "-fsanitize=address,undefined", str(probe), "-o", str(exe)], capture_output=True)
            if r.returncode == 0 and subprocess.run([str(exe)], capture_output=True, env=SANITIZER_ENV).returncode == 0:
                return cxx
    return None


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_host")
    cxx = sanitizer_compiler(tmp)
    if cxx is None:
        pytest.skip("no C++ compiler with the AddressSanitizer and UndefinedBehaviorSanitizer runtimes")
    exe = tmp / "jpeg_decode_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "audio2photoreal_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "jpeg_decode_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run_host(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=SANITIZER_ENV)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return r.stdout


def valid_files(images):
    """[(name, file bytes)]: every layout the GPU tests decode, small."""
    out = [(f"img_{s}_q{q}", J.encode(images[n], q, s)) for n, (s, q) in enumerate((("420", 10), ("444", 100), ("420", 90)))]
    img = images[2][:23, :37]
    for s in ("422", "gray", "420", "444"):
        cols = D.grid(23, 37, s)[1]
        out += [(f"lay_{s}_ri{ri}", D.encode(img, 75, s, ri, specs, dht))
                for ri, specs, dht in ((0, J.SPECS, True), (1, J.SPECS, True), (3, D.custom_specs(), True), (cols, J.SPECS, False), (999, J.SPECS, True))]
    rng = np.random.default_rng(3)
    for kind in ("worst", "runs", "only63", "dcswing", "stuffing"):
        coef = crafted(kind, (1, 2, 3, 6, 64), rng)[0]
        out.append((f"crafted_{kind}", D.encode_coefficients(coef, 32, 48, 90, "420", 3)))
    return out


def test_host_program_decodes_valid_streams_to_the_restatement_s_coefficients(host_program, images, tmp_path):
    files = valid_files(images)
    for name, data in files:
        (tmp_path / name).write_bytes(data)
    out = run_host(host_program, "decode", *[str(tmp_path / name) for name, _ in files])
    lines = out.strip().splitlines()
    assert len(lines) == len(files)
    for (name, data), line in zip(files, lines):
        assert f"{name} status=0 " in line, line
        _, want = D.decode_coefficients(data)
        got = np.fromfile(tmp_path / (name + ".coef"), np.int16).reshape(want.shape)
        assert np.array_equal(got, want), name


def test_host_program_rejects_the_designed_bad_streams_cleanly(host_program, images, tmp_path):
    """The inputs of the GPU rejection test, first: each is refused with its cause, with no sanitizer report."""
    bad = D.bad_streams(J.coefficients(images[0], 90, "420"), 40, 72)
    for name, (data, interval, cause) in bad.items():
        (tmp_path / name).write_bytes(data)
        out = run_host(host_program, "decode", str(tmp_path / name))
        assert f"status={interval << 4 | cause} " in out, (name, out)


def test_host_program_survives_seeded_corruptions(host_program, images, tmp_path):
    files = valid_files(images)
    paths = []
    for name, data in files[:3] + files[3::4]:
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    out = run_host(host_program, "fuzz", "20240611", "400", *paths)
    lines = out.strip().splitlines()
    assert len(lines) == len(paths)
    for line in lines:
        tally = {int(k): int(v) for k, v in re.findall(r"cause(\d+)=(\d+)", line)}
        assert sum(tally.values()) == 400 and set(tally) <= set(range(9)), line
        assert sum(v for k, v in tally.items() if k) > 100, line            # the corruptions are found, not slept through
