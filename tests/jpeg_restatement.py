"""Baseline JPEG (ITU-T T.81) and the RIFF AVI container restated in numpy from the standards, for the tests of audio2photoreal_amd/
video.py: the Annex K tables, the coefficient arithmetic of include/a2p_hip.h "video frames" in float64, an entropy encoder, a
baseline decoder (marker parser, Huffman decoding, restart intervals, dequantisation, float64 IDCT, chroma upsampling by
replication, inverse colour transform) and an AVI muxer / demuxer.  Nothing here imports the package under test."""
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------ tables
Q_LUMA = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
    [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101],
    [72, 92, 95, 98, 112, 100, 103, 99]])
Q_CHROMA = np.array([
    [17, 18, 24, 47, 99, 99, 99, 99], [18, 21, 26, 66, 99, 99, 99, 99], [24, 26, 56, 99, 99, 99, 99, 99], [47, 66, 99, 99, 99, 99, 99, 99],
    [99] * 8, [99] * 8, [99] * 8, [99] * 8])


def zigzag_order():
    """scan position -> natural index 8 v + u: the diagonals of Figure A.6, alternating direction."""
    out = []
    for s in range(15):
        diag = [(v, s - v) for v in range(8) if 0 <= s - v < 8]          # v ascending: down-left
        out += [8 * v + u for v, u in (diag if s % 2 else diag[::-1])]
    return out


ZIGZAG = zigzag_order()

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
SPECS = {"dc_luma": DC_LUMA, "ac_luma": AC_LUMA, "dc_chroma": DC_CHROMA, "ac_chroma": AC_CHROMA}
SPEC_IDS = {"dc_luma": 0x00, "ac_luma": 0x10, "dc_chroma": 0x01, "ac_chroma": 0x11}      # Tc << 4 | Th


def quant_tables(quality):
    """int [2, 8, 8]: the Annex K tables under libjpeg's quality scaling."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((t * s + 50) // 100, 1, 255) for t in (Q_LUMA, Q_CHROMA)])


def huffman_codes(bits, vals):
    """{symbol: (code, length)}: Annex C.2."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code *= 2
    return out


def layout(subsampling):
    """(MCU side, blocks per MCU) of "420" / "444"."""
    return {"420": (16, 6), "444": (8, 3)}[subsampling]


# ------------------------------------------------------------------------------------------------ test images
def source_images(height=40, width=72, seed=20240611):
    """uint8 [3, height, width, 3]: smooth, noise, mix (smooth plus N(0, 12))."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    smooth = np.stack([127 + 120 * np.sin(x / 9 + y / 5), 127 + 100 * np.cos(x / 4), (6 * y) % 256], -1)
    noise = rng.uniform(0, 255, size=smooth.shape)
    mix = smooth + rng.normal(0, 12, size=smooth.shape)
    return np.clip(np.rint(np.stack([smooth, noise, mix])), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


# ------------------------------------------------------------------------------------------------ coefficients, float64
def dct_matrix():
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0] /= np.sqrt(2.0)
    return c


def planes64(rgb, subsampling, dtype=np.float64):
    """(Y, Cb, Cr) float64 (or `dtype`), level-shifted, the image replicated at its right and bottom edge to whole MCUs, chroma the mean of 2 x 2
    groups for "420"."""
    mcu, _ = layout(subsampling)
    H, W, _ = rgb.shape
    Hp, Wp = -(-H // mcu) * mcu, -(-W // mcu) * mcu
    p = np.pad(rgb.astype(dtype), ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge")
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = -0.168735892 * R - 0.331264108 * G + 0.5 * B + 128
    Cr = 0.5 * R - 0.418687589 * G - 0.081312411 * B + 128
    if subsampling == "420":
        Cb, Cr = (c.reshape(Hp // 2, 2, Wp // 2, 2).mean((1, 3)) for c in (Cb, Cr))
    return Y - 128, Cb - 128, Cr - 128


def blocks_in_scan_order(Y, Cb, Cr, subsampling):
    """[mcu_rows, mcu_cols, blocks_per_mcu, 8, 8] (v, u natural) from three planes of any dtype."""
    mcu, bpm = layout(subsampling)
    rows, cols = Y.shape[0] // mcu, Y.shape[1] // mcu
    out = np.zeros((rows, cols, bpm, 8, 8), Y.dtype)
    for r in range(rows):
        for c in range(cols):
            k = 0
            for by in range(mcu // 8):
                for bx in range(mcu // 8):
                    out[r, c, k] = Y[r * mcu + 8 * by:r * mcu + 8 * by + 8, c * mcu + 8 * bx:c * mcu + 8 * bx + 8]
                    k += 1
            out[r, c, k] = Cb[8 * r:8 * r + 8, 8 * c:8 * c + 8]
            out[r, c, k + 1] = Cr[8 * r:8 * r + 8, 8 * c:8 * c + 8]
    return out


def quotients64(rgb, quality, subsampling, dtype=np.float64):
    """float64 [mcu_rows, mcu_cols, blocks_per_mcu, 64] in zig-zag order: F(u, v) / Q[v][u] before rounding; and the divisors.
    dtype=np.float32 runs the same steps in single precision (numpy's summation order, not the kernel's)."""
    blocks = blocks_in_scan_order(*planes64(rgb, subsampling, dtype), subsampling)
    C = dct_matrix().astype(dtype)
    F = np.einsum("vy,rckyx,ux->rckvu", C, blocks, C)
    q = quant_tables(quality).astype(dtype)
    ny = blocks.shape[2] - 2
    Q = np.stack([q[0]] * ny + [q[1]] * 2)
    shape = F.shape[:3] + (64,)
    return (F / Q).reshape(shape)[..., ZIGZAG], np.broadcast_to(Q.reshape(-1, 64)[:, ZIGZAG], shape)


def coefficients(rgb, quality, subsampling):
    """int16 in the layout of a2p_jpeg_coefficients: rint of the quotients, AC clamped to +-1023."""
    q = np.rint(quotients64(rgb, quality, subsampling)[0])
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q.astype(np.int16)


# ------------------------------------------------------------------------------------------------ entropy coding
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        assert 0 <= code < (1 << length)
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            self.out.append(self.acc >> self.n)
            self.acc &= (1 << self.n) - 1

    def flush(self):
        """Pads with 1-bits to a byte and stuffs a zero byte after every 0xFF."""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return bytes(self.out).replace(b"\xff", b"\xff\x00")


def _amplitude(v):
    """(size, bits) of F.1.2.1: size = bit length of |v|; negative values as v - 1 in `size` bits."""
    size = int(abs(int(v))).bit_length()
    return size, (int(v) if v >= 0 else int(v) - 1) & ((1 << size) - 1)


def encode_block(bits, zz, pred, dc_codes, ac_codes):
    """Codes the 64 coefficients `zz` (scan order) of one block after the DC predictor `pred`."""
    size, amp = _amplitude(int(zz[0]) - pred)
    bits.put(*dc_codes[size])
    bits.put(amp, size)
    run = 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac_codes[0xF0])
            run -= 16
        size, amp = _amplitude(zz[k])
        bits.put(*ac_codes[run << 4 | size])
        bits.put(amp, size)
        run = 0
    if run:
        bits.put(*ac_codes[0x00])


def entropy_segment(coef):
    """bytes: the entropy-coded segment of one frame's coefficients [mcu_rows, mcu_cols, blocks_per_mcu, 64] with one restart
    interval per MCU row."""
    codes = {k: huffman_codes(*v) for k, v in SPECS.items()}
    rows, cols, bpm, _ = coef.shape
    out = b""
    for r in range(rows):
        bits, pred = _Bits(), [0, 0, 0]
        for c in range(cols):
            for k in range(bpm):
                comp = 0 if k < bpm - 2 else k - (bpm - 2) + 1
                kind = "luma" if comp == 0 else "chroma"
                encode_block(bits, coef[r, c, k], pred[comp], codes["dc_" + kind], codes["ac_" + kind])
                pred[comp] = int(coef[r, c, k, 0])
        out += bits.flush()
        if r + 1 < rows:
            out += bytes([0xFF, 0xD0 + r % 8])
    return out


def _marker(code, payload):
    return bytes([0xFF, code]) + struct.pack(">H", len(payload) + 2) + payload


def header(height, width, quality, subsampling):
    """SOI, APP0 (JFIF 1.01, no density unit, 1 : 1), DQT 0 and 1, SOF0, DHT x 4, DRI, SOS."""
    mcu, _ = layout(subsampling)
    q = quant_tables(quality).reshape(2, 64)
    out = b"\xff\xd8" + _marker(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + struct.pack(">HH", 1, 1) + bytes([0, 0]))
    for i in range(2):
        out += _marker(0xDB, bytes([i]) + bytes(int(q[i][n]) for n in ZIGZAG))
    hv = 0x22 if subsampling == "420" else 0x11
    out += _marker(0xC0, bytes([8]) + struct.pack(">HH", height, width) + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for name in ("dc_luma", "ac_luma", "dc_chroma", "ac_chroma"):
        out += _marker(0xC4, bytes([SPEC_IDS[name]]) + bytes(SPECS[name][0]) + bytes(SPECS[name][1]))
    out += _marker(0xDD, struct.pack(">H", -(-width // mcu)))
    return out + _marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(rgb, quality, subsampling):
    """A complete JFIF file of one uint8 image [H, W, 3]."""
    return header(rgb.shape[0], rgb.shape[1], quality, subsampling) + entropy_segment(coefficients(rgb, quality, subsampling)) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ decoder
def parse(data):
    """The marker segments of a baseline file: {"dqt": {id: int [64] in scan order}, "dht": {Tc << 4 | Th: (bits, vals)}, "size": (H,
    W), "components": [(id, h, v, tq)], "dri": int, "scan": [(id, td, ta)], "segment": bytes (entropy-coded, up to EOI), "order":
    [marker codes in file order]}."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    out = {"dqt": {}, "dht": {}, "dri": 0, "order": [0xD8]}
    at = 2
    while True:
        assert data[at] == 0xFF, f"no marker at {at}"
        code, (length,) = data[at + 1], struct.unpack_from(">H", data, at + 2)
        body = data[at + 4:at + 2 + length]
        out["order"].append(code)
        if code == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "16-bit quantisation tables are not baseline"
                out["dqt"][body[0] & 15] = np.array(list(body[1:65]))
                body = body[65:]
        elif code == 0xC4:
            while body:
                bits = list(body[1:17])
                out["dht"][body[0]] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif code == 0xC0:
            assert body[0] == 8
            out["size"] = struct.unpack_from(">HH", body, 1)
            out["components"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
        elif code == 0xDD:
            out["dri"] = struct.unpack(">H", body)[0]
        elif code == 0xDA:
            out["scan"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            assert tuple(body[1 + 2 * body[0]:]) == (0, 63, 0), "not a sequential scan"
            end = data.rindex(b"\xff\xd9")
            out["segment"] = data[at + 2 + length:end]
            assert end + 2 == len(data), "bytes after EOI"
            out["order"].append(0xD9)
            return out
        else:
            assert code in (0xE0, 0xE1, 0xE2, 0xEE, 0xFE) or 0xE0 <= code <= 0xEF, f"marker {code:#x} is not baseline"
        at += 2 + length


def _intervals(segment):
    """The restart intervals of an entropy-coded segment with the stuffing removed; checks that RSTm counts 0..7 cyclically."""
    out, cur, i, m = [], bytearray(), 0, 0
    while i < len(segment):
        b = segment[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nxt = segment[i + 1]
        if nxt == 0:
            cur.append(0xFF)
        else:
            assert nxt == 0xD0 + m, f"marker {nxt:#x} where RST{m} is due"
            out.append(bytes(cur))
            cur, m = bytearray(), (m + 1) % 8
        i += 2
    return out + [bytes(cur)]


class _Reader:
    def __init__(self, data):
        self.value, self.n, self.at = int.from_bytes(data, "big") if data else 0, 8 * len(data), 0

    def bits(self, k):
        assert self.at + k <= self.n, "the interval ends inside a code"
        self.at += k
        return (self.value >> (self.n - self.at)) & ((1 << k) - 1)

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bits(1)
            if (length, code) in table:
                return table[length, code]
        raise AssertionError("no such Huffman code")

    def padding_is_ones(self):
        k = self.n - self.at
        return k < 8 and (k == 0 or self.bits(k) == (1 << k) - 1)


def _extend(bits, size):
    return bits if size == 0 or bits >> (size - 1) else bits - (1 << size) + 1


def decode_coefficients(data):
    """(parsed header, int [mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan order) of a baseline file whose luminance is sampled 2 x 2
    or 1 x 1 over 1 x 1 chrominance."""
    h = parse(data)
    comps = h["components"]
    assert len(comps) == 3 and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1) and comps[0][1] == comps[0][2] and comps[0][1] in (1, 2)
    ss = comps[0][1]
    mcu, bpm = 8 * ss, ss * ss + 2
    H, W = h["size"]
    rows, cols = -(-H // mcu), -(-W // mcu)
    tables = {k: {(l, c): s for s, (c, l) in huffman_codes(*v).items()} for k, v in h["dht"].items()}
    scan = {cid: (td, ta) for cid, td, ta in h["scan"]}
    per_block = [comps[0]] * (ss * ss) + [comps[1], comps[2]]
    ri = h["dri"] or rows * cols
    intervals = _intervals(h["segment"])
    assert len(intervals) == -(-rows * cols // ri), "the number of restart intervals"
    coef = np.zeros((rows * cols, bpm, 64), np.int64)
    for i, chunk in enumerate(intervals):
        rd, pred = _Reader(chunk), {c[0]: 0 for c in comps}
        for m in range(i * ri, min((i + 1) * ri, rows * cols)):
            for k, (cid, _, _, _) in enumerate(per_block):
                td, ta = scan[cid]
                size = rd.symbol(tables[td])
                pred[cid] += _extend(rd.bits(size), size)
                coef[m, k, 0] = pred[cid]
                j = 1
                while j < 64:
                    rs = rd.symbol(tables[0x10 | ta])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            break                      # EOB
                        j += 16
                        continue
                    j += run
                    assert j < 64, "a run past coefficient 63"
                    coef[m, k, j] = _extend(rd.bits(size), size)
                    j += 1
        assert rd.padding_is_ones(), "an interval is not padded with 1-bits to a byte"
    return h, coef.reshape(rows, cols, bpm, 64)


def decode(data):
    """uint8 [H, W, 3]: dequantisation, float64 IDCT, chroma replicated to the luminance grid, inverse colour transform, rounding."""
    h, coef = decode_coefficients(data)
    rows, cols, bpm, _ = coef.shape
    ss = h["components"][0][1]
    mcu = 8 * ss
    tq = [h["components"][0][3]] * (ss * ss) + [h["components"][1][3], h["components"][2][3]]
    Q = np.stack([h["dqt"][t] for t in tq]).astype(np.float64)
    nat = np.zeros((rows, cols, bpm, 64))
    nat[..., ZIGZAG] = coef * Q
    C = dct_matrix()
    px = np.clip(np.einsum("vy,rckvu,ux->rckyx", C, nat.reshape(rows, cols, bpm, 8, 8), C) + 128, 0, 255)   # A.3.1: samples are clamped
    Y = np.zeros((rows * mcu, cols * mcu))
    Cb, Cr = np.zeros((rows * 8, cols * 8)), np.zeros((rows * 8, cols * 8))
    for r in range(rows):
        for c in range(cols):
            for k in range(ss * ss):
                by, bx = divmod(k, ss)
                Y[r * mcu + 8 * by:r * mcu + 8 * by + 8, c * mcu + 8 * bx:c * mcu + 8 * bx + 8] = px[r, c, k]
            Cb[8 * r:8 * r + 8, 8 * c:8 * c + 8], Cr[8 * r:8 * r + 8, 8 * c:8 * c + 8] = px[r, c, bpm - 2], px[r, c, bpm - 1]
    Cb, Cr = (np.repeat(np.repeat(c, ss, 0), ss, 1) - 128 for c in (Cb, Cr))
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136286 * Cb - 0.714136286 * Cr, Y + 1.772 * Cb], -1)
    H, W = h["size"]
    return np.clip(np.rint(rgb[:H, :W]), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ AVI
def pcm16(audio):
    a = np.asarray(audio, np.float64)
    a = a[:, None] if a.ndim == 1 else a
    return np.rint(np.clip(a, -1, 1) * 32767).astype("<i2")


def _riff_chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + b"\0" * (len(payload) % 2)


def avi_mux(frames, height, width, fps, audio=None, audio_rate=None):
    """bytes of an AVI file: `frames` [bytes] as `00dc` chunks; `audio` int16 [samples, channels] as `01wb` chunks of one video second,
    each in front of that second's frames, the rest behind the last frame; `idx1` offsets count from the `movi` fourcc."""
    rate, scale = (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)
    chunks, done = [], 0
    n_audio = 0 if audio is None else len(audio)
    for i, f in enumerate(frames):
        second = i * scale // rate
        if audio is not None and (i == 0 or second != (i - 1) * scale // rate):
            b = min(n_audio, (second + 1) * audio_rate)
            if b > done:
                chunks.append((b"01wb", audio[done:b].tobytes()))
                done = b
        chunks.append((b"00dc", bytes(f)))
    while audio is not None and done < n_audio:
        b = min(n_audio, done + audio_rate)
        chunks.append((b"01wb", audio[done:b].tobytes()))
        done = b
    movi, index = b"movi", b""
    for fourcc, payload in chunks:
        index += fourcc + struct.pack("<III", 0x10, len(movi), len(payload))       # the first chunk sits 4 bytes behind the fourcc
        movi += _riff_chunk(fourcc, payload)
    big = lambda kind: max([len(p) for k, p in chunks if k == kind] or [0])
    n_streams = 1 if audio is None else 2
    bps = 0 if audio is None else audio_rate * audio.shape[1] * 2
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), int(big(b"00dc") * rate / scale) + bps, 0, 0x110, len(frames), 0, n_streams,
                       big(b"00dc"), width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, scale, rate, 0, len(frames), big(b"00dc"), -1, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _riff_chunk(b"avih", avih) + _riff_chunk(b"LIST", b"strl" + _riff_chunk(b"strh", strh) + _riff_chunk(b"strf", strf))
    if audio is not None:
        align = 2 * audio.shape[1]
        strh = b"auds" + struct.pack("<IIHHIIIIIIiI4h", 0, 0, 0, 0, 0, align, audio_rate * align, 0, n_audio, big(b"01wb"), -1, align, 0, 0, 0, 0)
        strf = struct.pack("<HHIIHHH", 1, audio.shape[1], audio_rate, audio_rate * align, align, 16, 0)
        hdrl += _riff_chunk(b"LIST", b"strl" + _riff_chunk(b"strh", strh) + _riff_chunk(b"strf", strf))
    body = b"AVI " + _riff_chunk(b"LIST", hdrl) + _riff_chunk(b"LIST", movi) + _riff_chunk(b"idx1", index)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def avi_demux(blob):
    """{"frames", "audio" (int16 [samples, channels] or None), "fps", "size" (height, width), "audio_rate", "chunks": [(fourcc, offset
    of the chunk header in the file, size)], "index": [(fourcc, flags, offset from the `movi` fourcc, size)], "movi": (offset of the
    `movi` fourcc, the list's size field), "riff_size"}; asserts the nesting is consistent."""
    blob = bytes(blob)
    assert blob[:4] == b"RIFF" and blob[8:12] == b"AVI "
    out = {"frames": [], "audio": None, "fps": None, "size": None, "audio_rate": None, "chunks": [], "index": [], "movi": None,
           "riff_size": struct.unpack_from("<I", blob, 4)[0], "streams": []}
    pcm, channels = [], [None]

    def walk(a, b, inside):
        while a < b:
            assert a + 8 <= b, "a chunk header runs past its list"
            fourcc, (size,) = blob[a:a + 4], struct.unpack_from("<I", blob, a + 4)
            body = a + 8
            assert body + size <= b, f"{fourcc} runs past its list"
            if fourcc == b"LIST":
                kind = blob[body:body + 4]
                if kind == b"movi":
                    out["movi"] = (body, size)
                walk(body + 4, body + size, kind)
            elif fourcc == b"avih":
                out["avih"] = struct.unpack_from("<14I", blob, body)
            elif fourcc == b"strh":
                out["streams"].append(blob[body:body + 4])
                if out["streams"][-1] == b"vids":
                    assert blob[body + 4:body + 8] == b"MJPG"
                    scale, rate, _, length = struct.unpack_from("<IIII", blob, body + 20)
                    out["fps"], out["video_length"] = rate / scale, length
                else:
                    out["audio_length"] = struct.unpack_from("<I", blob, body + 32)[0]
            elif fourcc == b"strf" and out["streams"][-1] == b"vids":
                w, h = struct.unpack_from("<ii", blob, body + 4)
                out["size"] = (h, w)
                assert blob[body + 16:body + 20] == b"MJPG"
            elif fourcc == b"strf":
                tag, channels[0], out["audio_rate"], _, align, width = struct.unpack_from("<HHIIHH", blob, body)
                assert (tag, width, align) == (1, 16, 2 * channels[0])
            elif fourcc == b"idx1":
                out["index"] = [(blob[i:i + 4],) + struct.unpack_from("<III", blob, i + 4) for i in range(body, body + size, 16)]
            elif inside == b"movi":
                out["chunks"].append((fourcc, a, size))
                (out["frames"] if fourcc == b"00dc" else pcm).append(blob[body:body + size])
                assert fourcc in (b"00dc", b"01wb")
            a = body + size + size % 2
        assert a == b, "padding runs past the list"

    walk(12, 8 + out["riff_size"], b"AVI ")
    if channels[0] is not None:
        out["audio"] = np.frombuffer(b"".join(pcm), "<i2").reshape(-1, channels[0]).copy()
    return out
