"""The cases of the JPEG encoder's tests: tests/test_gpu_jpeg_encode.py compares the device's bytes with tests/jpeg_encode_ref.py on
every one, tests/test_jpeg_encode_ref.py holds the definition itself to its round trip and to Pillow on the same list.  A reference file
is computed once per case and process (`reference`) and never changed.

Shapes are (h, w).  The default restart interval is 8 MCUs; what each case is there for stands behind it."""
import functools
import os

import numpy as np

from tests import jpeg_encode_ref as J

GOLDEN_PNG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_images", "sample_38x30.png")


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gradient(h, w, seed=1):
    """A smooth picture with a little noise: what a photograph looks like to the coder (few, small coefficients)."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1)
    return np.clip(base + np.random.default_rng(seed).integers(-8, 9, (h, w, 3)), 0, 255).astype(np.uint8)


def flat(h, w, value=(90, 160, 30)):
    return np.broadcast_to(np.array(value, dtype=np.uint8), (h, w, 3)).copy()


def checker_blocks(h, w):
    """8x8 blocks alternating 0 / 255 in both directions: the largest DC differences."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y // 8 + x // 8) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


ISOLATED = (17, 33, 49, 63)      # zigzag positions: zero runs of 16, 32, 48 (one, two, three ZRL) and a block that ends without an EOB


def isolated_coefficients():
    """A grey 8 x 32 image, one block per entry of ISOLATED: 128 + 400 x the DCT basis function of that position, so at quality 50 the
    luma block has a DC of 0, exactly one nonzero AC coefficient, at that position, and the chroma blocks are empty."""
    k = np.arange(8)
    blocks = []
    for z in ISOLATED:
        u, v = divmod(int(J.ZIGZAG[z]), 8)
        basis = np.outer(np.cos((2 * k + 1) * u * np.pi / 16), np.cos((2 * k + 1) * v * np.pi / 16))
        blocks.append(np.rint(128 + 400 * 0.25 * basis))
    return np.repeat(np.clip(np.concatenate(blocks, axis=1), 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def _cases():
    out = {}

    def add(name, image, quality, subsampling, interval=None):
        assert name not in out
        out[name] = (image, quality, subsampling, interval)
    for sub in J.SUBSAMPLINGS:
        # shapes: less than a block, one block, one 4:2:0 MCU, padding on both axes, odd on both, many segments (RSTm wraps past 7)
        for h, w in ((1, 1), (8, 8), (16, 16), (17, 9), (33, 47), (24, 200)):
            add(f"shape-{h}x{w}-{sub}", (gradient(h, w).astype(int) // 2 + noise(h, w, 3) // 2).astype(np.uint8), 75, sub)
        for q in (1, 50, 95, 100):          # (75: the shapes above); noise at 100: the longest codes and dense 0xFF stuffing
            add(f"noise-q{q}-{sub}", noise(33, 47, q), q, sub)
        add(f"flat-{sub}", flat(40, 24), 50, sub)                       # EOB only, DC differences 0 after the first block
        add(f"isolated-{sub}", isolated_coefficients(), 50, sub)        # ZRL runs of 1, 2, 3; no EOB
        add(f"checker-{sub}", checker_blocks(32, 48), 100, sub)         # the largest DC differences
        add(f"photo-{sub}", gradient(21, 53), 95, sub)
    add("interval5-444", noise(16, 72, 7), 75, "444", 5)               # 9 MCUs a row, 18 MCUs: segments cross rows, the last one is short
    add("interval3-420", gradient(40, 56), 90, "420", 3)               # 4 x 3 MCUs: four whole segments
    add("one-whole-segment-420", noise(16, 128, 8), 75, "420", 8)      # exactly 8 MCUs = one segment, no RSTm at all
    add("one-short-segment-444", gradient(8, 24), 75, "444", 65535)    # 3 MCUs, the largest interval
    add("interval1-444", noise(24, 40, 9), 95, "444", 1)               # 15 segments of one MCU: every DC is a difference from 0
    add("several-workgroups-420", gradient(360, 640), 95, "420")       # 920 MCUs, 115 segments: the scan over segment lengths
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference(name) -> bytes:
    image, quality, subsampling, interval = CASES[name]
    return J.encode_jpeg_np(image, quality, subsampling, interval)
