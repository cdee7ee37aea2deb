"""CPU: the numpy definition of the PNG encoder (tests/png_encode_ref.py) against Pillow, zlib and the test's own decoder: every file is
valid (all CRCs, the zlib stream, the Adler-32), decodes to exactly the input, every filter type and every block form occurs in the case
set, the code construction keeps its limits, and the size stays within a stated excess over Pillow and over zlib's Z_RLE."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_encode_cases as JK
from tests import png_encode_cases as K
from tests import png_encode_ref as P

# The size gates: twice the largest excess measured on the images of `_size_images` (the table of DESIGN "PNG encode").  Small images
# are judged in bytes (the 75 fixed bytes and the 12 + ~60 bytes of chunk framing and code description per segment dominate), the
# 256x256 ones by relative excess.  Measured: Pillow arm 58 bytes (flat 64x48) and 0.4987 (flat 256x256: 1,139 bytes against 760);
# Z_RLE arm 81 bytes and 0.7909 (the same flat image, against 636 bytes).
PILLOW_GATE_BYTES, PILLOW_GATE_RELATIVE = 116, 0.9974
ZRLE_GATE_BYTES, ZRLE_GATE_RELATIVE = 162, 1.5818


def _pillow_bytes(image) -> int:
    out = io.BytesIO()
    Image.fromarray(image).save(out, "PNG", compress_level=6)
    return len(out.getvalue())


def _zrle_bytes(image) -> int:
    """zlib level 6 with Z_RLE on the same filtered stream: the deflate stream alone."""
    f, _ = P.filter_rows(image)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(f.tobytes()) + c.flush())


def _size_images():
    small = {"sample 38x30": K.golden(), "gradient + noise 64x48": JK.gradient(64, 48), "noise 33x47": JK.noise(33, 47), "flat 64x48": K.flat(64, 48)}
    large = {"gradient + noise 256x256": JK.gradient(256, 256), "noise 256x256": JK.noise(256, 256), "flat 256x256": K.flat(256, 256),
             "speckled flat 256x256": K.speckled(256, 256)}
    return small, large


@pytest.mark.parametrize("name", list(K.CASES))
def test_file_is_valid_and_lossless(name):
    image, segment_bytes = K.CASES[name]
    data, d = K.reference(name), K.details(name)
    Image.open(io.BytesIO(data)).verify()                       # every CRC
    h, w, c = image.shape
    if image.dtype == np.uint8 or c == 1:                        # what Pillow reads back exactly
        got = np.asarray(Image.open(io.BytesIO(data)))
        assert got.dtype == image.dtype or c == 1 and image.dtype == np.uint16
        assert np.array_equal(got.reshape(h, w, c).astype(image.dtype), image)
    decoded, stream = P.decode_png_np(data)                      # the test's own reader, for all six formats
    assert decoded.dtype == image.dtype and np.array_equal(decoded, image)
    assert np.array_equal(stream, d["stream"]) and len(stream) == h * (1 + w * c * image.dtype.itemsize)
    chunks = P.parse_chunks(data)
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (len(d["segments"]) + 2) + [b"IEND"]
    assert chunks[1][1] == b"\x78\x01" and [body for _, body in chunks[2:-2]] == d["segments"]
    assert chunks[-2][1] == struct.pack(">I", zlib.adler32(stream.tobytes()))
    s = segment_bytes or P.DEFAULT_SEGMENT_BYTES
    assert len(d["segments"]) == (len(stream) + s - 1) // s
    assert len(data) == 47 + sum(12 + len(x) for x in d["segments"]) + 28 <= P.max_bytes_np(h, w, c, 8 * image.dtype.itemsize, s)
    assert data[:47] == P.header_np(h, w, c, 8 * image.dtype.itemsize)


def test_every_filter_and_every_block_form_occurs():
    types, forms = set(), set()
    for name in K.CASES:
        d = K.details(name)
        types |= set(d["types"].tolist())
        forms |= {("last-" if i == len(d["kinds"]) - 1 else "") + kind for i, kind in enumerate(d["kinds"])}
    assert types == {0, 1, 2, 3, 4}
    assert forms == {"dynamic", "stored", "last-dynamic", "last-stored"}


def test_filter_choice_is_the_smallest_cost_lowest_type_first():
    image = K.CASES["gradient-33x47-c3-8"][0]
    f, types = P.filter_rows(image)
    rows = image.reshape(33, -1).astype(np.int64)
    for y in (0, 1, 17, 32):
        up = rows[y - 1] if y else np.zeros_like(rows[0])
        left, upleft = np.concatenate([[0, 0, 0], rows[y][:-3]]), np.concatenate([[0, 0, 0], up[:-3]])
        p = left + up - upleft
        pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        costs = [int(np.abs(((rows[y] - pred) & 255).astype(np.uint8).view(np.int8).astype(np.int64)).sum())
                 for pred in (0, left, up, (left + up) // 2, paeth)]
        assert types[y] == costs.index(min(costs)) and f[y, 0] == types[y]


def test_tokens_are_the_rule_position_by_position():
    for name, (stream, s) in K.STREAM_CASES.items():
        for k in range(0, len(stream), s):
            assert P.tokens(stream[k:k + s]) == P.tokens_slow(stream[k:k + s]), (name, k)
    for name in ("speckled-c3-8-s64", "flat-c4-16-s100", "one-byte-last-segment"):
        stream, s = K.details(name)["stream"], K.CASES[name][1]
        for k in range(0, len(stream), s):
            assert P.tokens(stream[k:k + s]) == P.tokens_slow(stream[k:k + s]), (name, k)


def test_the_run_lengths_end_at_a_segments_last_byte():
    stream, s = K.STREAM_CASES["runs-s600"]
    tails = []
    for k in range(0, len(stream) - 1, s):
        seg = stream[k:k + s]
        tails.append(int(s - 1 - np.flatnonzero(seg[:-1] != seg[-1]).max()) if (seg != seg[-1]).any() else s)
    assert tuple(tails) == K.RUN_LENGTHS + (s,) and len(stream) % s == 1
    toks = P.tokens(stream[:s])            # a run of 2 behind its first byte: literals only
    assert toks[-2:] == [7, 7] and all(t >= 0 for t in toks)
    assert P.tokens(stream[3 * s:4 * s])[-2:] == [7, -256]            # 257 = literal + match 256
    assert P.tokens(stream[5 * s:6 * s])[-2:] == [7, -258]            # 259
    assert P.tokens(stream[6 * s:7 * s])[-3:] == [7, -258, 7]         # 260: one byte is left over
    assert P.tokens(stream[8 * s:9 * s])[-3:] == [7, -258, -258]      # 517
    assert P.tokens(stream[9 * s:10 * s]) == [7, -258, -258, -83]     # a whole segment of one byte: 1 + 258 + 258 + 83 = 600


@pytest.mark.parametrize("name", list(K.STREAM_CASES))
def test_zlib_reads_the_bare_stream(name):
    stream, _ = K.STREAM_CASES[name]
    assert zlib.decompress(K.stream_reference(name)) == stream.tobytes()


def fibonacci(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def code_count_cases():
    rs = np.random.default_rng(4)
    out = {"random-286": (rs.integers(0, 2000, 286).tolist(), 15), "random-sparse": ((rs.integers(0, 50, 286) * (rs.random(286) < 0.3)).tolist(), 15),
           "random-19": (rs.integers(0, 40, 19).tolist(), 7),
           # Fibonacci counts 1, 1, 2, 3 ...: the unlimited tree is a chain.  Over 286 symbols the sequence restarts every 40 symbols
           # (F(40) = 102,334,155: the sum of all counts stays below 2^32, the kernel's word)
           "fibonacci-286": ([fibonacci(40)[i % 40] for i in range(286)], 15), "fibonacci-40-of-286": (fibonacci(40) + [0] * 246, 15),
           "fibonacci-19": (fibonacci(19), 7),
           "one-symbol": ([0] * 100 + [5] + [0] * 185, 15), "one-symbol-19": ([0, 0, 3] + [0] * 16, 7), "none": ([0] * 286, 15),
           "all-equal-286": ([3] * 286, 15), "all-equal-19": ([1] * 19, 7), "all-equal-256": ([9] * 256 + [0] * 30, 15), "two": ([0, 4, 0, 4] + [0] * 15, 7)}
    return out


@pytest.mark.parametrize("name", list(code_count_cases()))
def test_build_lengths_keeps_the_limit_and_is_complete(name):
    counts, limit = code_count_cases()[name]
    lengths = P.build_lengths(counts, limit)
    used = [(c, l) for c, l in zip(counts, lengths) if c]
    assert all(l == 0 for c, l in zip(counts, lengths) if not c) and all(1 <= l <= limit for _, l in used)
    if len(used) == 1:
        assert used[0][1] == 1
    elif used:
        assert sum(1 << (limit - l) for _, l in used) == 1 << limit            # the Kraft sum is exactly 1
        by_count = sorted(used, key=lambda u: (u[0], -u[1]))
        assert all(a[1] >= b[1] for a, b in zip(by_count, by_count[1:]))         # a more frequent symbol never has the longer code
    if name.startswith("fibonacci"):
        assert max(P.huffman_depths(sorted(c for c in counts if c))) > limit      # the limit bites
    if name.startswith("random") and len(used) > 1:                               # no limit in the way: the cost is Huffman's
        depths = P.huffman_depths(sorted(c for c in counts if c))
        if max(depths) <= limit:
            assert sum(c * l for c, l in used) == sum(c * d for c, d in zip(sorted(c for c in counts if c), depths))


def test_size_against_pillow_and_zlib_rle(capsys):
    small, large = _size_images()
    lines, worst = [], {"pb": 0, "pr": 0.0, "zb": 0, "zr": 0.0}
    for group, images in (("small", small), ("large", large)):
        for name, image in images.items():
            ours, pillow, zrle = len(P.encode_png_np(image)), _pillow_bytes(image), _zrle_bytes(image)
            lines.append(f"{name}: ours {ours}, Pillow level 6 {pillow} ({ours - pillow:+d} bytes, x{ours / pillow:.4f}), "
                         f"zlib level 6 Z_RLE stream {zrle} ({ours - zrle:+d} bytes, x{ours / zrle:.4f})")
            if group == "small":
                worst["pb"], worst["zb"] = max(worst["pb"], ours - pillow), max(worst["zb"], ours - zrle)
            else:
                worst["pr"], worst["zr"] = max(worst["pr"], ours / pillow - 1), max(worst["zr"], ours / zrle - 1)
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\nlargest excess: {worst}")
    assert worst["pb"] <= PILLOW_GATE_BYTES and worst["pr"] <= PILLOW_GATE_RELATIVE, worst
    assert worst["zb"] <= ZRLE_GATE_BYTES and worst["zr"] <= ZRLE_GATE_RELATIVE, worst


def test_refusals_of_the_definition():
    with pytest.raises(ValueError, match="uint8 or uint16"):
        P.encode_png_np(np.zeros((4, 4, 3), np.int32))
    with pytest.raises(ValueError, match="c in 1, 3, 4"):
        P.encode_png_np(np.zeros((4, 4, 2), np.uint8))
    for bad in (63, 65536, -1):
        with pytest.raises(ValueError, match="segment_bytes"):
            P.encode_png_np(np.zeros((4, 4, 3), np.uint8), bad)
