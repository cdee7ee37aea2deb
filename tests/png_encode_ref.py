"""The definition of the device PNG encoder (csrc/png_encode.hip; DESIGN "PNG encode"), in numpy and Python integers only.  The kernels
meet `encode_png_np` byte for byte; Pillow and zlib judge validity, losslessness and size, never the bytes.

    F        the filtered stream: per row one filter-type byte (libpng's heuristic: the smallest sum of |int8(byte)| over None, Sub, Up,
             Average, Paeth; ties to the lowest type) and the row's filtered bytes; 16-bit samples big-endian.  T = h (1 + w bpp) bytes.
    segments F[k S : (k + 1) S], S = segment_bytes (64..65535, default 16384): one deflate block each, no reference across a start.
    tokens   literals and distance-1 matches, greedy from the left inside the segment (`tokens`).
    codes    `build_lengths`: one deterministic length-limited construction for the literal/length code (limit 15) and for the
             code-length code (limit 7); canonical codes per RFC 1951 3.2.2.
    block    dynamic, followed by an empty stored block unless it is the last one; or, when that is not smaller, one stored block.
    file     47 constant bytes (signature, IHDR, an IDAT with the zlib header 78 01), one IDAT per segment, an IDAT with the Adler-32,
             IEND.

`decode_png_np` is the test's own decoder for the files Pillow cannot read back exactly (16-bit RGB and RGBA)."""
import struct
import zlib

import numpy as np

DEFAULT_SEGMENT_BYTES = 16384
HEADER_BYTES = 47
COLOUR_TYPES = {1: 0, 3: 2, 4: 6}
LIT_LIMIT, CL_LIMIT = 15, 7
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
LENGTH_SYMBOL = {}          # match length 3..258 -> (symbol, extra bits, extra value): the largest base not above the length
for _l in range(3, 259):
    _k = max(k for k in range(29) if LENGTH_BASE[k] <= _l)
    LENGTH_SYMBOL[_l] = (257 + _k, LENGTH_EXTRA[_k], _l - LENGTH_BASE[_k])


def check_image(image, segment_bytes):
    image = np.asarray(image)
    if image.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"encode_png_np: uint8 or uint16 samples, got {image.dtype}")
    if image.ndim == 2:
        image = image[..., None]
    if image.ndim != 3 or image.shape[2] not in COLOUR_TYPES or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"encode_png_np: an [h,w] or [h,w,c] image with c in 1, 3, 4 and h, w >= 1, got {image.shape}")
    if segment_bytes is not None and segment_bytes != 0 and not 64 <= segment_bytes <= 65535:
        raise ValueError(f"encode_png_np: segment_bytes must be None, 0 or in 64..65535, got {segment_bytes!r}")
    return image, segment_bytes or DEFAULT_SEGMENT_BYTES


# ---- the filtered stream ----
def stream_bytes(image):
    """[h,w,c] uint8 / uint16 -> the rows as PNG stores them, uint8 [h, w * bpp] (16-bit samples big-endian), and bpp."""
    h, w, c = image.shape
    if image.dtype == np.uint16:
        rows = np.stack([image >> 8, image & 255], -1).astype(np.uint8).reshape(h, w * c * 2)
        return rows, 2 * c
    return image.reshape(h, w * c), c


def filter_rows(image):
    """-> (F uint8 [h, 1 + w bpp], the chosen types int [h])."""
    rows, bpp = stream_bytes(image)
    h, rb = rows.shape
    x = rows.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if rb > bpp else 0          # left
    b = np.zeros_like(x)
    b[1:] = x[:-1]                                        # up
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if rb > bpp else 0        # up left
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))          # the specification's tie order: a, then b, then c
    filtered = np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]) & 255        # [5, h, rb]
    cost = np.where(filtered < 128, filtered, 256 - filtered).sum(axis=2)           # sum of |int8|
    types = np.argmin(cost, axis=0)                       # the first smallest: ties to the lowest type
    out = np.empty((h, 1 + rb), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = filtered[types, np.arange(h)]
    return out, types


# ---- tokens ----
def tokens(seg):
    """The greedy rule on one segment (uint8 [n]) -> list of literals (0..255) and matches (-length): at i >= 1 with seg[i] == seg[i-1],
    L = the run of that byte from i, capped at 258 and the segment end; L >= 3: a match (L, 1), else a literal."""
    out, i, n = [], 0, len(seg)
    change = np.flatnonzero(seg[1:] != seg[:-1]) + 1
    ends = np.append(change, n)                           # the end of the maximal run that each start begins
    starts = np.append(0, change)
    for s, e in zip(starts.tolist(), ends.tolist()):
        byte = int(seg[s])
        out.append(byte)                                  # a run's first byte differs from the byte before it (or starts the segment)
        i = s + 1
        while i < e:
            length = min(e - i, 258)
            if length >= 3:
                out.append(-length)
                i += length
            else:
                out.append(byte)
                i += 1
    return out


def tokens_slow(seg):
    """The rule exactly as the issue words it, position by position (the test holds `tokens` to it)."""
    out, i, n = [], 0, len(seg)
    while i < n:
        if i >= 1 and seg[i] == seg[i - 1]:
            length = 0
            while i + length < n and length < 258 and seg[i + length] == seg[i]:
                length += 1
            if length >= 3:
                out.append(-length)
                i += length
                continue
        out.append(int(seg[i]))
        i += 1
    return out


# ---- the length-limited code ----
def huffman_depths(weights):
    """Leaf depths of the Huffman tree over `weights` (ascending, at least two): two queues, leaves and merged nodes in creation order;
    of a leaf and a node of equal weight the LEAF is taken first."""
    n = len(weights)
    node_w, leaf_parent, node_parent = [0] * (n - 1), [0] * n, [0] * (n - 1)
    li = ni = 0
    for k in range(n - 1):
        total = 0
        for _ in range(2):
            if li < n and (ni >= k or weights[li] <= node_w[ni]):
                total += weights[li]
                leaf_parent[li] = k
                li += 1
            else:
                total += node_w[ni]
                node_parent[ni] = k
                ni += 1
        node_w[k] = total
    depth = [0] * (n - 1)
    for j in range(n - 3, -1, -1):
        depth[j] = depth[node_parent[j]] + 1
    return [depth[p] + 1 for p in leaf_parent]


def build_lengths(counts, limit):
    """counts [nsym] -> code lengths [nsym], 0 for a count of 0.
      1. the used symbols sorted ascending by (count, symbol);
      2. no used symbol: all 0; one: that symbol gets length 1;
      3. `huffman_depths`; depths above `limit` count as `limit`; per length the number of codes;
      4. the repair: while the Kraft sum (in units of 2^-limit) exceeds 1: take one code away from `limit`, and turn one code of the
         longest length below `limit` that has any into two codes one bit longer (the sum falls by exactly one unit per round);
      5. lengths go out by rank: the most frequent symbol (the LAST of the sorted list) gets the shortest length, and so on down."""
    counts = [int(c) for c in counts]
    order = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    lengths = [0] * len(counts)
    if len(order) <= 1:
        for _, s in order:
            lengths[s] = 1
        return lengths
    per_length = [0] * (limit + 1)
    for d in huffman_depths([c for c, _ in order]):
        per_length[min(d, limit)] += 1
    total = sum(per_length[i] << (limit - i) for i in range(1, limit + 1))
    while total > 1 << limit:
        per_length[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if per_length[i]:
                per_length[i] -= 1
                per_length[i + 1] += 2
                break
        total -= 1
    j = len(order)
    for length in range(1, limit + 1):
        for _ in range(per_length[length]):
            j -= 1
            lengths[order[j][1]] = length
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> per symbol the code, already BIT-REVERSED for the LSB-first stream."""
    top = max(lengths) if len(lengths) else 0
    per_length = [0] * (top + 2)
    for length in lengths:
        per_length[length] += 1
    per_length[0] = 0
    code, next_code = 0, [0] * (top + 2)
    for bits in range(1, top + 1):
        code = (code + per_length[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for length in lengths:
        if length:
            out.append(int(format(next_code[length], f"0{length}b")[::-1], 2))
            next_code[length] += 1
        else:
            out.append(0)
    return out


def cl_tokens(seq):
    """Code lengths -> (symbol, extra value) of the code-length alphabet, greedy from the left: a run of zeros from here of 11 or more is
    one 18 (up to 138), of 3..10 one 17; a nonzero value equal to the one before it whose run from here is 3 or more is one 16 (up to 6);
    everything else is the value itself."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            run = min(run, 138)
            out.append((18, run - 11))
        elif v == 0 and run >= 3:
            out.append((17, run - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and run >= 3:
            run = min(run, 6)
            out.append((16, run - 3))
        else:
            run = 1
            out.append((v, 0))
        i += run
    return out


class BitWriter:
    """Deflate's packing: bits fill every byte from its least significant end."""

    def __init__(self):
        self.acc = self.n = 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        self.align()
        return self.acc.to_bytes(self.n // 8, "little")


def deflate_segment(seg, last):
    """One segment (uint8 [n], 1 <= n <= 65535) -> (its deflate bytes, "dynamic" or "stored")."""
    n = len(seg)
    toks = tokens(seg)
    counts = [0] * 286
    for t in toks:
        counts[t if t >= 0 else LENGTH_SYMBOL[-t][0]] += 1
    counts[256] = 1
    lit_len = build_lengths(counts, LIT_LIMIT)
    hlit = max(s for s in range(286) if lit_len[s]) + 1          # (>= 257: the end of block is always used)
    seq = lit_len[:hlit] + [1]                                   # ... and the one distance code, symbol 0 of length 1
    cl = cl_tokens(seq)
    cl_counts = [0] * 19
    for s, _ in cl:
        cl_counts[s] += 1
    cl_len = build_lengths(cl_counts, CL_LIMIT)
    hclen = max(max(k for k in range(19) if cl_len[CL_ORDER[k]]) + 1, 4)
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl_len[s] + CL_EXTRA.get(s, 0) for s, _ in cl)
    bits += sum(counts[s] * lit_len[s] for s in range(286))
    bits += sum(counts[257 + k] * (LENGTH_EXTRA[k] + 1) for k in range(29))          # extra bits and the 1-bit distance code
    dynamic_bytes = (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4
    if dynamic_bytes >= 5 + n:
        return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(seg), "stored"
    w = BitWriter()
    w.put(1 if last else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_len[CL_ORDER[k]], 3)
    cl_code = canonical_codes(cl_len)
    for s, extra in cl:
        w.put(cl_code[s], cl_len[s])
        if s in CL_EXTRA:
            w.put(extra, CL_EXTRA[s])
    code = canonical_codes(lit_len)
    for t in toks:
        if t >= 0:
            w.put(code[t], lit_len[t])
        else:
            s, extra_bits, extra = LENGTH_SYMBOL[-t]
            w.put(code[s], lit_len[s])
            w.put(extra, extra_bits)
            w.put(0, 1)                                          # distance 1: the only distance code, one bit, no extra bits
    w.put(code[256], lit_len[256])
    assert w.n == bits, (w.n, bits)
    if not last:
        w.put(0, 3)                                              # an empty stored block: 000, pad to the byte, 00 00 FF FF
        w.align()
        w.put(0xFFFF0000, 32)
    out = w.bytes()
    assert len(out) == dynamic_bytes
    return out, "dynamic"


def deflate_stream(stream, segment_bytes=DEFAULT_SEGMENT_BYTES):
    """uint8 [T] -> (the segments' deflate bytes, their kinds)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8).reshape(-1)
    k = (len(stream) + segment_bytes - 1) // segment_bytes
    done = [deflate_segment(stream[i * segment_bytes:(i + 1) * segment_bytes], i == k - 1) for i in range(k)]
    return [d for d, _ in done], [kind for _, kind in done]


def zlib_stream_np(stream, segment_bytes=DEFAULT_SEGMENT_BYTES):
    """A bare zlib stream of `stream`: 78 01, the segments, the Adler-32 (what resr_png_debug_deflate returns)."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8).reshape(-1)
    return b"\x78\x01" + b"".join(deflate_stream(stream, segment_bytes)[0]) + struct.pack(">I", zlib.adler32(stream.tobytes()))


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def header_np(h, w, channels, depth):
    """The 47 bytes every file starts with."""
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, COLOUR_TYPES[channels], 0, 0, 0))
            + chunk(b"IDAT", b"\x78\x01"))


def max_bytes_np(h, w, channels, depth, segment_bytes=None):
    t = h * (1 + w * channels * depth // 8)
    s = segment_bytes or DEFAULT_SEGMENT_BYTES
    return t + 17 * ((t + s - 1) // s) + 75


def encode_png_np(image, segment_bytes=None, details=None):
    """[h,w] or [h,w,c] uint8 / uint16, c in 1, 3, 4 -> the file.  `details` (a dict) receives F, the filter types and the block kinds."""
    image, s = check_image(image, segment_bytes)
    h, w, c = image.shape
    f, types = filter_rows(image)
    flat = f.reshape(-1)
    segments, kinds = deflate_stream(flat, s)
    if details is not None:
        details.update(stream=flat, types=types, kinds=kinds, segments=segments)
    out = header_np(h, w, c, 8 * image.dtype.itemsize) + b"".join(chunk(b"IDAT", d) for d in segments)
    out += chunk(b"IDAT", struct.pack(">I", zlib.adler32(flat.tobytes()))) + chunk(b"IEND", b"")
    assert len(out) == HEADER_BYTES + sum(12 + len(d) for d in segments) + 28 <= max_bytes_np(h, w, c, 8 * image.dtype.itemsize, s)
    return out


# ---- the test's own reader ----
def parse_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1] == (b"IEND", b"")
    return out


def decode_png_np(data):
    """A file of colour type 0, 2 or 6, 8 or 16 bits, not interlaced -> (the image [h,w,c], the filtered stream F)."""
    chunks = parse_chunks(data)
    w, h, depth, colour, compression, flt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert chunks[0][0] == b"IHDR" and (compression, flt, interlace) == (0, 0, 0)
    c = {v: k for k, v in COLOUR_TYPES.items()}[colour]
    bpp = c * depth // 8
    f = np.frombuffer(zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT")), dtype=np.uint8).reshape(h, 1 + w * bpp)
    rows = np.zeros((h + 1, bpp + w * bpp), dtype=np.int64)      # a zero row above, bpp zero bytes to the left
    for y in range(h):
        kind, cur, up = int(f[y, 0]), rows[y + 1], rows[y]
        for x in range(bpp, bpp + w * bpp):
            a, b, cc = cur[x - bpp], up[x], up[x - bpp]
            p = a + b - cc
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
            pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else b if pb <= pc else cc)[kind]
            cur[x] = (int(f[y, x - bpp + 1]) + pred) & 255
    body = rows[1:, bpp:].astype(np.uint8)
    if depth == 16:
        pairs = body.reshape(h, w, c, 2).astype(np.uint16)
        return (pairs[..., 0] << 8 | pairs[..., 1]), f.reshape(-1)
    return body.reshape(h, w, c), f.reshape(-1)
