"""The definition of the device JPEG encoder (csrc/jpeg_encode.hip, include/resr.h "JPEG encode"), in numpy, integers only.

`encode_jpeg_np(rgb, quality, subsampling, restart_interval)` is the whole file, byte for byte what the kernels write.  Baseline JPEG
(JFIF 1.01, sequential DCT, 8 bits, YCbCr, Huffman); the rules, in the order the data meets them:

COLOUR.  JFIF full-range BT.601 in Q16, one rounding.  With R, G, B the bytes of a pixel,
    Y  = ( 19595 R + 38470 G +  7471 B                + 32768) >> 16
    Cb = (-11059 R - 21709 G + 32768 B + (128 << 16)  + 32767) >> 16
    Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16)  + 32767) >> 16          (>> floors)
  The Y constants add up to 65536 and each chroma row to 0, so (v, v, v) gives Y = v and Cb = Cr = 128 exactly.  No clamp is needed: Y
  is at most (255 * 65536 + 32768) >> 16 = 255; a chroma value lies in 128 +- 127.5 before rounding and the rounding term is one short
  of a half, so the extremes are floor(255.99998) = 255 and floor(0.99998) = 0.
SUBSAMPLING.  "444": a chroma sample per pixel, MCU 8x8, blocks Y Cb Cr.  "420" (h2v2): a chroma sample per 2x2 pixels, MCU 16x16,
  blocks Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr.  The box mean is taken of R, G, B BEFORE the colour rule, as exact sums SR, SG, SB of the four
  pixels, and rounded once, with the colour rule two bits wider:
    Cb = (-11059 SR - 21709 SG + 32768 SB + (128 << 18) + 131071) >> 18,   Cr likewise
  (one rounding, no bias of a second one; the same no-clamp argument holds).  An image whose sides are no multiple of the MCU is padded
  by replicating its last row / column (of RGB, before anything else).
DCT.  Samples s = level - 128.  C[u][x] = rint(0.5 alpha(u) cos((2x + 1) u pi / 16) 2^20), alpha(0) = 1 / sqrt 2, else 1 (Q20).
    T[u][x] = sum_y C[u][y] s[y][x]          exact; |T| <= 128 * 2.83 * 2^20 < 2^29: int32
    F[u][v] = sum_x C[v][x] T[u][x]          exact; |F| < 2^51: int64 (Q40).  u is the vertical frequency, v the horizontal.
    G[u][v] = (F + 2^26) >> 27               Q13, |G| < 2^24: int32
QUANTISATION.  Annex K base tables, IJG quality rule: scale = 5000 // q below 50 else 200 - 2 q; step = clamp((base * scale + 50) // 100,
  1, 255).  coefficient = sign(G) * ((|G| + (step << 12)) // (step << 13)): G / (step 2^13) rounded half away from zero.
ENTROPY.  Zigzag order; DC difference per component, predictor 0 at the start of every restart segment; AC (run, size) symbols with ZRL
  (0xF0) for runs over 15 and EOB (0x00) unless coefficient 63 is nonzero; the four Annex K "typical" tables; a negative value v of
  size s is sent as v - 1 in s bits.  Bits are packed MSB first, a 0xFF byte is followed by 0x00, the last byte of a segment is padded
  with 1-bits (a padded byte that becomes 0xFF is stuffed too).
RESTART.  restart_interval > 0: a DRI segment in the header, a segment per `restart_interval` MCUs (MCUs in raster order), RSTm
  (0xFFD0 + m, m = segment index mod 8) between segments.  0: no DRI, one segment (the device encoder never does this; it is here to
  measure what the markers cost).  None: DEFAULT_RESTART_INTERVAL.
FILE.  SOI, APP0 (JFIF 1.01, density 1:1, no units), DQT (two 8-bit tables in one segment), SOF0, DHT (four tables in one segment),
  DRI, SOS, the scan, EOI.

`decode_scan_np(file)` is a test-side Huffman decoder: it reads the tables out of the FILE's own DHT segment and returns the quantised
coefficients [mcus, blocks per MCU, 64] in zigzag order, so the entropy coder is checked without Pillow and without this file's tables.
"""
import numpy as np

DEFAULT_RESTART_INTERVAL = 8

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                     dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, dtype=np.int64)
# ZIGZAG[z] = natural (row-major, row = vertical frequency) index of the z-th coefficient
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFFMAN = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)      # in DHT order: classes / ids 0x00, 0x10, 0x01, 0x11
SUBSAMPLINGS = ("444", "420")


def dct_matrix() -> np.ndarray:
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    alpha = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
    return np.rint(0.5 * alpha * np.cos((2 * x + 1) * u * np.pi / 16) * (1 << 20)).astype(np.int64)


def quant_tables(quality: int) -> np.ndarray:
    """int64 [2, 64] steps (luma, chroma) in natural order."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be 1..100, got {quality!r}")
    scale = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    return np.clip((np.stack([BASE_LUMA, BASE_CHROMA]) * scale + 50) // 100, 1, 255)


def _check(rgb, subsampling):
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or min(rgb.shape) < 1 or max(rgb.shape[:2]) > 65535:
        raise ValueError(f"expected an HxWx3 uint8 image with sides 1..65535, got {rgb.dtype} {rgb.shape}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    return rgb


def samples_np(rgb, subsampling):
    """The level-shifted samples of every block: int64 [mcus_y, mcus_x, blocks per MCU, 8, 8]."""
    rgb = _check(rgb, subsampling)
    m = 16 if subsampling == "420" else 8
    h, w = rgb.shape[:2]
    p = np.pad(rgb, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    my, mx = p.shape[0] // m, p.shape[1] // m
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    if subsampling == "420":
        r, g, b = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] for c in (r, g, b))
        shift = 18
    else:
        shift = 16
    half = (1 << (shift - 1)) - 1
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << shift) + half) >> shift
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << shift) + half) >> shift

    def blocks(plane):      # [my * k * 8, mx * k * 8] -> [my, mx, k * k, 8, 8], the k x k blocks of an MCU in raster order
        k = plane.shape[0] // (my * 8)
        return plane.reshape(my, k, 8, mx, k, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, k * k, 8, 8)
    return np.concatenate([blocks(y), blocks(cb), blocks(cr)], axis=2) - 128


def dct_q13_np(samples):
    """G of the docstring for blocks [..., 8, 8] (y, x) -> [..., 8, 8] (u, v), int64."""
    c = dct_matrix()
    t = np.einsum("uy,...yx->...ux", c, samples)
    f = np.einsum("vx,...ux->...uv", c, t)
    return (f + (1 << 26)) >> 27


def quantise_np(g, steps):
    """G [..., 64] natural order, steps [64] or broadcastable -> coefficients, half away from zero."""
    return np.sign(g) * ((np.abs(g) + (steps << 12)) // (steps << 13))


def frontend_np(rgb, quality, subsampling):
    """The quantised coefficients the entropy coder sends: int64 [mcus, blocks per MCU, 64] in ZIGZAG order, MCUs in raster order."""
    s = samples_np(rgb, subsampling)
    my, mx, nb = s.shape[:3]
    g = dct_q13_np(s).reshape(my * mx, nb, 64)
    q = quant_tables(quality)
    steps = np.stack([q[0]] * (nb - 2) + [q[1], q[1]])          # [nb, 64]
    return quantise_np(g, steps)[..., ZIGZAG]


def huffman_codes(bits, vals):
    """symbol -> (code, length) of a (bits, vals) table, the canonical assignment of Annex C."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def _segment(marker, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header_np(h, w, quality, subsampling, restart_interval) -> bytes:
    """SOI .. SOS."""
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, b"".join(bytes([i]) + bytes(q[i][ZIGZAG].astype(np.uint8)) for i in range(2)))
    samp = 0x22 if subsampling == "420" else 0x11
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    out += _segment(0xC4, b"".join(bytes([tc]) + bytes(bits) + bytes(vals) for tc, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFFMAN)))
    if restart_interval:
        out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _encode_block(bits, z, pred, dc, ac):
    """One block (zigzag coefficients z) after a predictor `pred`; returns the new predictor."""
    diff = int(z[0]) - pred
    size = abs(diff).bit_length()
    bits.put(*dc[size])
    if size:
        bits.put((diff if diff > 0 else diff - 1) & ((1 << size) - 1), size)
    last = 0
    for k in np.flatnonzero(z[1:]) + 1:
        v, run = int(z[k]), int(k) - 1 - last
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        size = abs(v).bit_length()
        bits.put(*ac[run << 4 | size])
        bits.put((v if v > 0 else v - 1) & ((1 << size) - 1), size)
        last = int(k)
    if last != 63:
        bits.put(*ac[0x00])
    return int(z[0])


def resolve_interval(restart_interval):
    r = DEFAULT_RESTART_INTERVAL if restart_interval is None else restart_interval
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r <= 65535:
        raise ValueError(f"restart_interval must be None or 0..65535, got {restart_interval!r}")
    return int(r)


def scan_np(coefs, restart_interval) -> bytes:
    """The entropy-coded scan (with its RSTm markers) of frontend_np's coefficients."""
    dcs = [huffman_codes(*DC_LUMA), huffman_codes(*DC_CHROMA)]
    acs = [huffman_codes(*AC_LUMA), huffman_codes(*AC_CHROMA)]
    n, nb = coefs.shape[:2]
    comp = [0] * (nb - 2) + [1, 2]
    per = restart_interval or n
    out = bytearray()
    for seg, first in enumerate(range(0, n, per)):
        if seg:
            out += bytes([0xFF, 0xD0 + (seg - 1) % 8])
        bits, pred = _Bits(), [0, 0, 0]
        for m in range(first, min(first + per, n)):
            for b in range(nb):
                c = comp[b]
                pred[c] = _encode_block(bits, coefs[m, b], pred[c], dcs[min(c, 1)], acs[min(c, 1)])
        bits.flush()
        out += bits.out
    return bytes(out)


def encode_jpeg_np(rgb, quality=95, subsampling="420", restart_interval=None) -> bytes:
    rgb = _check(rgb, subsampling)
    r = resolve_interval(restart_interval)
    return header_np(rgb.shape[0], rgb.shape[1], quality, subsampling, r) + scan_np(frontend_np(rgb, quality, subsampling), r) + b"\xff\xd9"


# ---- the test-side decoder of the scan ----
def parse_np(data: bytes):
    """The segments of a file of this encoder: dict with h, w, sampling (0x11 / 0x22), interval, tables {(class, id): (bits, vals)},
    quant {id: [64] zigzag}, scan (the bytes between SOS and EOI)."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9", "no SOI / EOI"
    info, at = {"interval": 0, "tables": {}, "quant": {}}, 2
    while True:
        assert data[at] == 0xFF, f"no marker at {at}"
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            for k in range(0, len(body), 65):
                info["quant"][body[k]] = list(body[k + 1:k + 65])
        elif marker == 0xC0:
            info["h"], info["w"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            info["sampling"] = body[7]
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                bits = list(body[k + 1:k + 17])
                info["tables"][(body[k] >> 4, body[k] & 15)] = (bits, list(body[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        elif marker == 0xDD:
            info["interval"] = int.from_bytes(body, "big")
        elif marker == 0xDA:
            info["scan"] = data[at:-2]
            return info


def decode_scan_np(data: bytes) -> np.ndarray:
    info = parse_np(data)
    m = 16 if info["sampling"] == 0x22 else 8
    nb = 6 if info["sampling"] == 0x22 else 3
    n = -(-info["h"] // m) * -(-info["w"] // m)
    lookup = {key: {(length, code): sym for sym, (code, length) in huffman_codes(*t).items()} for key, t in info["tables"].items()}
    comp = [0] * (nb - 2) + [1, 2]
    per = info["interval"] or n
    scan, out = info["scan"], np.zeros((n, nb, 64), dtype=np.int64)
    # split at the RSTm markers (a 0xFF followed by 0x00 is data), then unstuff
    segments, start, k = [], 0, 0
    while k < len(scan) - 1:
        if scan[k] == 0xFF and scan[k + 1] != 0:
            assert scan[k + 1] == 0xD0 + len(segments) % 8, f"marker {scan[k + 1]:#x} where RST{len(segments) % 8} belongs"
            segments.append(scan[start:k])
            start = k = k + 2
        else:
            k += 2 if scan[k] == 0xFF else 1
    segments.append(scan[start:])
    assert len(segments) == -(-n // per), f"{len(segments)} segments for {n} MCUs at interval {per}"
    for seg, raw in enumerate(segments):
        raw = raw.replace(b"\xff\x00", b"\xff")
        value, nbits, pos = int.from_bytes(raw, "big"), 8 * len(raw), 0

        def take(count):
            nonlocal pos
            v = (value >> (nbits - pos - count)) & ((1 << count) - 1) if count else 0
            pos += count
            return v

        def symbol(table):
            code = 0
            for length in range(1, 17):
                code = code << 1 | take(1)
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError("no Huffman code matches")

        def signed(size):
            v = take(size)
            return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1

        pred = [0, 0, 0]
        for mcu in range(seg * per, min((seg + 1) * per, n)):
            for b in range(nb):
                c = comp[b]
                pred[c] += signed(symbol(lookup[(0, min(c, 1))]))
                out[mcu, b, 0] = pred[c]
                k = 1
                while k < 64:
                    sym = symbol(lookup[(1, min(c, 1))])
                    if sym == 0:
                        break
                    k += sym >> 4
                    if sym & 15:
                        out[mcu, b, k] = signed(sym & 15)
                    k += 1
                assert k <= 64, "a run past the end of the block"
        rest = nbits - pos
        assert 0 <= rest < 8 and take(rest) == (1 << rest) - 1, "the padding of a segment must be 1-bits of less than a byte"
    return out
