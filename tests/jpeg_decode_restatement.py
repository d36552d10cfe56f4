"""jpeg_restatement's numpy encoder and decoder generalised for the tests of the GPU decoder (audio2photoreal_amd/video.py
decode_jpeg_frames): 4:2:2 and grayscale beside 4:2:0 and 4:4:4, any restart interval (0: none), caller-supplied Huffman tables, and
files without DHT (the AVI MJPEG convention: the Annex K tables are implied).  Float64 throughout; nothing here imports the package
under test.  tests/test_video_decode_cpu.py pins it to jpeg_restatement.decode / decode_coefficients on every file those accept."""
import struct

import numpy as np

import jpeg_restatement as J

LAYOUTS = {"444": (1, 1, 3), "422": (2, 1, 3), "420": (2, 2, 3), "gray": (1, 1, 1)}      # luma h, luma v, components


def layout(sampling):
    """(luma h, luma v, components, blocks per MCU)."""
    hs, vs, nc = LAYOUTS[sampling]
    return hs, vs, nc, 1 if nc == 1 else hs * vs + 2


def grid(height, width, sampling):
    hs, vs, _, bpm = layout(sampling)
    return -(-height // (8 * vs)), -(-width // (8 * hs)), bpm


# ------------------------------------------------------------------------------------------------ Huffman tables that are not Annex K
def custom_specs():
    """Valid tables unlike the standard's: DC with codes of 3, 4, 5 and one of 16 bits (category 11); AC with 128 codes of 8 bits, 33
    of 9 and one of 16 bits, which is the commonest symbol of all (run 0, size 1), so that nearly every block holds a 16-bit code."""
    dc_bits = [0, 0, 4, 4, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    ac_bits = [0, 0, 0, 0, 0, 0, 0, 128, 33, 0, 0, 0, 0, 0, 0, 1]
    return {"dc_luma": (dc_bits, [5, 4, 3, 6, 2, 7, 1, 8, 0, 9, 10, 11]), "dc_chroma": (dc_bits, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 10]),
            "ac_luma": (ac_bits, J.AC_LUMA[1][::-1]), "ac_chroma": (ac_bits, [s for s in J.AC_CHROMA[1][::-1] if s != 0x01] + [0x01])}


# ------------------------------------------------------------------------------------------------ encoder
def planes64(rgb, sampling):
    """(Y, Cb, Cr) float64, level-shifted, padded by edge replication to whole MCUs, chroma the mean of luma h x luma v groups."""
    hs, vs, nc, _ = layout(sampling)
    H, W, _ = rgb.shape
    Hp, Wp = -(-H // (8 * vs)) * 8 * vs, -(-W // (8 * hs)) * 8 * hs
    p = np.pad(rgb.astype(np.float64), ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge")
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168735892 * R - 0.331264108 * G + 0.5 * B + 128
    Cr = 0.5 * R - 0.418687589 * G - 0.081312411 * B + 128
    Cb, Cr = (c.reshape(Hp // vs, vs, Wp // hs, hs).mean((1, 3)) for c in (Cb, Cr))
    return Y - 128, Cb - 128, Cr - 128


def blocks_in_scan_order(Y, Cb, Cr, sampling):
    hs, vs, nc, bpm = layout(sampling)
    rows, cols = Y.shape[0] // (8 * vs), Y.shape[1] // (8 * hs)
    out = np.zeros((rows, cols, bpm, 8, 8))
    for r in range(rows):
        for c in range(cols):
            k = 0
            for by in range(vs):
                for bx in range(hs):
                    y, x = (r * vs + by) * 8, (c * hs + bx) * 8
                    out[r, c, k] = Y[y:y + 8, x:x + 8]
                    k += 1
            if nc == 3:
                out[r, c, k], out[r, c, k + 1] = Cb[8 * r:8 * r + 8, 8 * c:8 * c + 8], Cr[8 * r:8 * r + 8, 8 * c:8 * c + 8]
    return out


def coefficients(rgb, quality, sampling):
    """int16 [mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan order: rint of F / Q, AC clamped to +-1023."""
    hs, vs, nc, bpm = layout(sampling)
    blocks = blocks_in_scan_order(*planes64(rgb, sampling), sampling)
    C = J.dct_matrix()
    F = np.einsum("vy,rckyx,ux->rckvu", C, blocks, C)
    q = J.quant_tables(quality).astype(np.float64)
    Q = np.stack([q[0]] * (bpm if nc == 1 else bpm - 2) + [q[1]] * (0 if nc == 1 else 2))
    out = np.rint((F / Q).reshape(F.shape[:3] + (64,))[..., J.ZIGZAG])
    out[..., 1:] = np.clip(out[..., 1:], -1023, 1023)
    return out.astype(np.int16)


def entropy_segment(coef, ri, specs=J.SPECS):
    """The entropy-coded segment of coefficients [mcu_rows, mcu_cols, bpm, 64] with a restart interval of `ri` MCUs (0: none)."""
    codes = {k: J.huffman_codes(*v) for k, v in specs.items()}
    rows, cols, bpm, _ = coef.shape
    ny = 1 if bpm == 1 else bpm - 2
    flat = coef.reshape(rows * cols, bpm, 64)
    ri = ri or len(flat)
    out, m = b"", 0
    for i, a in enumerate(range(0, len(flat), ri)):
        bits, pred = J._Bits(), [0, 0, 0]
        for mcu in flat[a:a + ri]:
            for k in range(bpm):
                comp = 0 if k < ny else k - ny + 1
                kind = "luma" if comp == 0 else "chroma"
                J.encode_block(bits, mcu[k], pred[comp], codes["dc_" + kind], codes["ac_" + kind])
                pred[comp] = int(mcu[k, 0])
        out += bits.flush()
        if a + ri < len(flat):
            out += bytes([0xFF, 0xD0 + i % 8])
    return out


def header(height, width, quality, sampling, ri, specs=J.SPECS, dht=True):
    hs, vs, nc, _ = layout(sampling)
    q = J.quant_tables(quality).reshape(2, 64)
    out = b"\xff\xd8" + J._marker(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + struct.pack(">HH", 1, 1) + bytes([0, 0]))
    for i in range(1 if nc == 1 else 2):
        out += J._marker(0xDB, bytes([i]) + bytes(int(q[i][n]) for n in J.ZIGZAG))
    comps = [1, hs << 4 | vs, 0] + ([2, 0x11, 1, 3, 0x11, 1] if nc == 3 else [])
    out += J._marker(0xC0, bytes([8]) + struct.pack(">HH", height, width) + bytes([nc] + comps))
    if dht:
        for name in ("dc_luma", "ac_luma") + (("dc_chroma", "ac_chroma") if nc == 3 else ()):
            out += J._marker(0xC4, bytes([J.SPEC_IDS[name]]) + bytes(specs[name][0]) + bytes(specs[name][1]))
    if ri:
        out += J._marker(0xDD, struct.pack(">H", ri))
    return out + J._marker(0xDA, bytes([nc, 1, 0x00] + ([2, 0x11, 3, 0x11] if nc == 3 else []) + [0, 63, 0]))


def encode_coefficients(coef, height, width, quality, sampling, ri, specs=J.SPECS, dht=True):
    """A complete file around given coefficients [mcu_rows, mcu_cols, bpm, 64]."""
    assert dht or specs is J.SPECS, "a file without DHT implies the Annex K tables"
    return header(height, width, quality, sampling, ri, specs, dht) + entropy_segment(coef, ri, specs) + b"\xff\xd9"


def encode(rgb, quality, sampling, ri=None, specs=J.SPECS, dht=True):
    """A complete file of one uint8 image [H, W, 3]; ri=None: one MCU row, as the GPU encoder writes."""
    H, W, _ = rgb.shape
    ri = grid(H, W, sampling)[1] if ri is None else ri
    return encode_coefficients(coefficients(rgb, quality, sampling), H, W, quality, sampling, ri, specs, dht)


# ------------------------------------------------------------------------------------------------ decoder
ANNEX_K = {J.SPEC_IDS[k]: (list(v[0]), list(v[1])) for k, v in J.SPECS.items()}


def parse(data):
    """jpeg_restatement.parse, with the Annex K tables standing in when the file has no DHT, and "sampling"."""
    h = J.parse(data)
    if not h["dht"]:
        h["dht"] = dict(ANNEX_K)
    comps = h["components"]
    assert len(comps) in (1, 3)
    if len(comps) == 1:
        h["sampling"] = "gray"
    else:
        assert comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1)
        h["sampling"] = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[comps[0][1:3]]
    return h


def decode_coefficients(data):
    """(parsed header, int [mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan order)."""
    h = parse(data)
    comps = h["components"]
    hs, vs, nc, bpm = layout(h["sampling"])
    rows, cols, _ = grid(*h["size"], h["sampling"])
    tables = {k: {(l, c): s for s, (c, l) in J.huffman_codes(*v).items()} for k, v in h["dht"].items()}
    scan = {cid: (td, ta) for cid, td, ta in h["scan"]}
    per_block = [comps[0]] * (bpm if nc == 1 else bpm - 2) + list(comps[1:])
    ri = h["dri"] or rows * cols
    intervals = J._intervals(h["segment"])
    assert len(intervals) == -(-rows * cols // ri), "the number of restart intervals"
    coef = np.zeros((rows * cols, bpm, 64), np.int64)
    for i, chunk in enumerate(intervals):
        rd, pred = J._Reader(chunk), {c[0]: 0 for c in comps}
        for m in range(i * ri, min((i + 1) * ri, rows * cols)):
            for k, (cid, _, _, _) in enumerate(per_block):
                td, ta = scan[cid]
                size = rd.symbol(tables[td])
                pred[cid] += J._extend(rd.bits(size), size)
                coef[m, k, 0] = pred[cid]
                j = 1
                while j < 64:
                    rs = rd.symbol(tables[0x10 | ta])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            break
                        j += 16
                        continue
                    j += run
                    assert j < 64, "a run past coefficient 63"
                    coef[m, k, j] = J._extend(rd.bits(size), size)
                    j += 1
        assert rd.padding_is_ones(), "an interval is not padded with 1-bits to a byte"
    return h, coef.reshape(rows, cols, bpm, 64)


def pixels64(h, coef):
    """float64 [H, W, 3] before rounding: dequantisation, IDCT, + 128 and the clamp of A.3.1, chroma replicated over its luma h x
    luma v group, the inverse colour transform."""
    rows, cols, bpm, _ = coef.shape
    hs, vs, nc, _ = layout(h["sampling"])
    ny = bpm if nc == 1 else bpm - 2
    tq = [h["components"][0][3]] * ny + [c[3] for c in h["components"][1:]]
    Q = np.stack([h["dqt"][t] for t in tq]).astype(np.float64)
    nat = np.zeros((rows, cols, bpm, 64))
    nat[..., J.ZIGZAG] = coef * Q
    C = J.dct_matrix()
    px = np.clip(np.einsum("vy,rckvu,ux->rckyx", C, nat.reshape(rows, cols, bpm, 8, 8), C) + 128, 0, 255)
    Y = np.zeros((rows * 8 * vs, cols * 8 * hs))
    Cb, Cr = np.zeros((rows * 8, cols * 8)), np.zeros((rows * 8, cols * 8))
    for r in range(rows):
        for c in range(cols):
            for k in range(ny):
                by, bx = divmod(k, hs)
                y, x = (r * vs + by) * 8, (c * hs + bx) * 8
                Y[y:y + 8, x:x + 8] = px[r, c, k]
            if nc == 3:
                Cb[8 * r:8 * r + 8, 8 * c:8 * c + 8], Cr[8 * r:8 * r + 8, 8 * c:8 * c + 8] = px[r, c, bpm - 2], px[r, c, bpm - 1]
    H, W = h["size"]
    if nc == 1:
        return np.stack([Y, Y, Y], -1)[:H, :W]
    Cb, Cr = (np.repeat(np.repeat(c, vs, 0), hs, 1) - 128 for c in (Cb, Cr))
    return np.stack([Y + 1.402 * Cr, Y - 0.344136286 * Cb - 0.714136286 * Cr, Y + 1.772 * Cb], -1)[:H, :W]


def decode(data):
    """uint8 [H, W, 3]."""
    return np.clip(np.rint(pixels64(*decode_coefficients(data))), 0, 255).astype(np.uint8)


def check_pixels(got, exact, delta=1e-3):
    """The pixel rule of the GPU tests: got (uint8) equals rint(exact) (float64 before rounding, then clamped) except where exact lies
    within delta of a half-integer; there it may differ by 1, never by more.  Returns (share of pixels inside the band, mismatches)."""
    want = np.clip(np.rint(exact), 0, 255)
    band = np.abs(exact - np.floor(exact) - 0.5) < delta
    diff = got.astype(np.int64) - want.astype(np.int64)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    assert not diff[~band].any(), (int(np.count_nonzero(diff[~band])), int(np.abs(diff).max()))
    assert np.abs(diff).max(initial=0) <= 1
    return float(band.mean()), int(np.count_nonzero(diff))


# ------------------------------------------------------------------------------------------------ designed rejections
def bad_streams(good_coef, height, width, sampling="420"):
    """{name: (file bytes, failing interval, cause code of include/a2p_hip.h)}: files the decoder must reject by design, built around
    valid coefficients with one restart interval per MCU row (at least 3 rows)."""
    rows, cols, bpm, _ = good_coef.shape
    assert rows >= 3
    head = header(height, width, 90, sampling, cols)
    seg = entropy_segment(good_coef, cols)
    marks = [i for i in range(len(seg) - 1) if seg[i] == 0xFF and 0xD0 <= seg[i + 1] <= 0xD7]
    out = {}
    # the file ends in the middle of the second interval, without EOI: one marker where rows - 1 are due
    out["truncated"] = (head + seg[:marks[0] + 2 + (marks[1] - marks[0]) // 2].rstrip(b"\xff"), 1, 1)
    swapped = bytearray(seg)
    swapped[marks[0] + 1], swapped[marks[1] + 1] = swapped[marks[1] + 1], swapped[marks[0] + 1]
    out["rst_order"] = (head + bytes(swapped) + b"\xff\xd9", 0, 2)
    # a code in no table: Annex K's DC luminance table has no code that starts with nine 1-bits; 0xFF 0x00 0xFF 0x00 is sixteen
    first = seg[:marks[0]]
    out["no_code"] = (head + b"\xff\x00\xff\x00" + seg[len(first):] + b"\xff\xd9", 0, 4)
    # a run past 63: one block of DC 0 followed by four ZRL (j = 65 is accepted silently: no coefficient) would pass, so code
    # (run 15, size 1) five times: j = 1 + 5 * 16 > 63 at the fourth
    codes = {k: J.huffman_codes(*v) for k, v in J.SPECS.items()}
    bits = J._Bits()
    bits.put(*codes["dc_luma"][0])
    for _ in range(5):
        bits.put(*codes["ac_luma"][0xF1])
        bits.put(1, 1)
    out["run_past_63"] = (head + bits.flush() + seg[len(first):] + b"\xff\xd9", 0, 5)
    out["ends_in_code"] = (head + first[:max(2, len(first) // 2)].rstrip(b"\xff") + seg[len(first):] + b"\xff\xd9", 0, 6)
    return out
