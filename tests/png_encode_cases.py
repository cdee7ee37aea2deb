"""The cases of the PNG encoder's tests: tests/test_gpu_png_encode.py compares the device's bytes with tests/png_encode_ref.py on every
one, tests/test_png_encode_ref.py holds the definition itself to Pillow, zlib and its own decoder on the same list.  A reference is
computed once per case and process (`reference`, `stream_reference`) and never changed.

CASES: name -> (image [h,w,c] uint8 / uint16, segment_bytes or None).  STREAM_CASES: name -> (bytes uint8 [T], segment_bytes): streams
for resr_png_debug_deflate, which skips the filter stage, so that the runs are exactly the ones written here."""
import functools
import os

import numpy as np
from PIL import Image

from tests import png_encode_ref as P
from tests.jpeg_encode_cases import gradient as _gradient_rgb

GOLDEN_PNG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_images", "sample_38x30.png")
SIZES = ((1, 1), (1, 7), (7, 1), (33, 47), (38, 30), (64, 48))
FORMATS = tuple((c, d) for d in (8, 16) for c in (1, 3, 4))
RUN_LENGTHS = (2, 3, 4, 257, 258, 259, 260, 516, 517)


def golden():
    return np.array(Image.open(GOLDEN_PNG).convert("RGB"))


def to_format(rgb, c, depth, seed=0):
    """An RGB uint8 picture as c channels of `depth` bits: grey = the green channel, alpha = a ramp; 16 bits = the byte twice plus noise
    in the low byte (so both bytes of a sample matter)."""
    h, w = rgb.shape[:2]
    planes = {1: rgb[..., 1:2], 3: rgb, 4: np.concatenate([rgb, (np.mgrid[0:h, 0:w][1] * 255 // max(w - 1, 1)).astype(np.uint8)[..., None]], -1)}[c]
    if depth == 8:
        return np.ascontiguousarray(planes)
    low = np.random.default_rng(seed).integers(0, 4, planes.shape).astype(np.uint16)
    return (planes.astype(np.uint16) << 8 | planes) ^ low


def noise(h, w, c=3, depth=8, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << depth, (h, w, c)).astype(np.uint8 if depth == 8 else np.uint16)


def gradient(h, w, c=3, depth=8, seed=1):
    return to_format(_gradient_rgb(h, w, seed), c, depth, seed)


def flat(h, w, c=3, depth=8):
    value = np.array([90, 160, 30, 200][:c] if depth == 8 else [0x5A5A, 0xA0A0, 0x1E1E, 0xC8C8][:c])
    return np.broadcast_to(value.astype(np.uint8 if depth == 8 else np.uint16), (h, w, c)).copy()


def speckled(h, w, c=3, depth=8, seed=3):
    """Flat rectangles with sparse speckle: the "anime" picture of the issue's table."""
    rs = np.random.default_rng(seed)
    image = flat(h, w, c, depth)
    image[h // 3:, w // 2:] = image[0, 0] // 2
    image[: h // 2, w // 4: w // 2] = image[0, 0] // 3 + 7
    hits = rs.random((h, w)) < 0.02
    image[hits] = rs.integers(0, 1 << depth, (int(hits.sum()), c)).astype(image.dtype)
    return image


def run_stream(segment_bytes):
    """One segment per entry of RUN_LENGTHS (twice: once behind a different byte, once filling the tail behind noise that ends in the
    run's own byte, so that the run is one longer than written), each ending in a run of exactly that length at the segment's last byte;
    then a segment that is one run from end to end and a one-byte last segment."""
    rs = np.random.default_rng(5)
    parts = []
    for length in RUN_LENGTHS:
        head = rs.integers(1, 255, segment_bytes - length, dtype=np.uint8)
        head[1:][head[1:] == head[:-1]] ^= 0x55          # no accidental runs in the head
        head[-1] = 200 if head[-2] != 200 else 201
        parts += [head, np.full(length, 7, np.uint8)]
    parts += [np.full(segment_bytes, 7, np.uint8), np.array([7], np.uint8)]
    return np.concatenate(parts)


def _cases():
    out = {}
    for (h, w) in SIZES:
        for c, depth in FORMATS:
            base = golden() if (h, w) == (38, 30) else _gradient_rgb(h, w)
            out[f"gradient-{h}x{w}-c{c}-{depth}"] = (to_format(base, c, depth), 64 if (h, w) == (33, 47) else None)
    for c, depth in FORMATS:
        out[f"flat-c{c}-{depth}-s100"] = (flat(33, 47, c, depth), 100)              # runs past 258 and across segment boundaries
        out[f"noise-c{c}-{depth}-s100"] = (noise(33, 47, c, depth, 2), 100)         # stored blocks, the last one too
        out[f"speckled-c{c}-{depth}-s64"] = (speckled(64, 48, c, depth), 64)
    out["flat-default"] = (flat(64, 48), None)
    out["speckled-default"] = (speckled(64, 48), None)
    out["noise-default"] = (noise(64, 48), None)
    out["rows-are-segments"] = (golden(), 1 + golden().shape[1] * 3)      # segment_bytes divides T: one row per segment
    out["divides-33x47"] = (gradient(33, 47), 142)
    out["one-byte-last-segment"] = (speckled(64, 48), 1031)                         # T = 64 * 145 = 9 * 1031 + 1
    out["noise-then-flat"] = (np.concatenate([noise(16, 48), flat(48, 48)]), 512)   # stored segments, then dynamic ones, a dynamic last
    out["flat-then-noise"] = (np.concatenate([flat(48, 48), noise(16, 48)]), 512)   # ... a stored last
    out["largest-segment"] = (speckled(64, 48), 65535)
    return out


CASES = _cases()
STREAM_CASES = {
    "runs-s600": (run_stream(600), 600),
    "runs-s64": (np.concatenate([np.full(61, 9, np.uint8), np.array([1, 1, 1], np.uint8), np.full(64, 1, np.uint8), np.array([1, 2], np.uint8)]), 64),
    "noise-s100": (np.random.default_rng(9).integers(0, 256, 1001, dtype=np.uint8), 100),
}


@functools.lru_cache(maxsize=None)
def reference(name) -> bytes:
    image, segment_bytes = CASES[name]
    return P.encode_png_np(image, segment_bytes)


@functools.lru_cache(maxsize=None)
def details(name) -> dict:
    image, segment_bytes = CASES[name]
    d = {}
    P.encode_png_np(image, segment_bytes, d)
    return d


@functools.lru_cache(maxsize=None)
def stream_reference(name) -> bytes:
    return P.zlib_stream_np(*STREAM_CASES[name])
