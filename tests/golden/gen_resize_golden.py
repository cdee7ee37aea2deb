"""Writes tests/golden/image_resize_native.npz: inputs and the reference's own `image_resize` outputs for the native resize kernel
(csrc/image_resize.hip), the (length, scale) pairs at which the reference raises, and `_resize_matrix` values to pin.

    python tests/golden/gen_resize_golden.py

Needs the reference (tests/golden/ref_shim.py); the tests read only the .npz.  Inputs are image-like fp32 [3,H,W] arrays that
overshoot [0, 1] as an unclamped SR output does: tests/golden/dataset_images/sample_38x30.png enlarged (bicubic), plus sigma 0.03
noise (fixed seed), rounded to values float16 holds exactly (they are stored and used as float32; the file compresses)."""
import hashlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_shim  # noqa: E402

CASES = [(120, 152, 0.5), (117, 150, 0.75), (92, 100, 0.375), (60, 76, 0.625), (40, 52, 1.5), (4, 4, 0.5), (8, 8, 0.375), (2, 2, 1.5),
         (3, 40, 0.625)]
RAISE_SCALES = [0.5, 0.75, 0.375, 0.625, 1.5, 0.25, 0.125, 2.0, 3.0, 1 / 3, 0.9, 1.25, 0.3]
MATRICES = [(120, 0.5, True), (117, 0.75, True), (92, 0.375, True), (60, 0.625, True), (40, 1.5, True), (152, 0.5, False), (8, 0.375, True),
            (4, 0.5, True), (2, 1.5, True), (40, 0.625, True)]


def sample_image(h, w, seed):
    from PIL import Image
    png = np.asarray(Image.open(os.path.join(HERE, "dataset_images", "sample_38x30.png")).convert("RGB")).astype(np.float32) / 255.0
    t = torch.from_numpy(png.transpose(2, 0, 1))[None]
    big = torch.nn.functional.interpolate(t, size=(h, w), mode="bicubic", align_corners=False)[0]
    noise = torch.randn(big.shape, generator=torch.Generator().manual_seed(seed)) * 0.03
    return (big + noise).half().float().numpy()


def main():
    ref = ref_shim.load("imgproc")
    from real_esrgan_pytorch_amd import imgproc
    out = {"cases": np.array(CASES, dtype=np.float64)}
    for i, (h, w, r) in enumerate(CASES):
        x = sample_image(h, w, seed=100 + i)
        y = ref.image_resize(torch.from_numpy(x), r).numpy()
        assert y.shape == (3, math.ceil(h * r), math.ceil(w * r)) and y.dtype == np.float32
        out[f"in_{i}"], out[f"out_{i}"] = x, y
        print(f"case {i}: {h}x{w} x {r} -> {y.shape[1]}x{y.shape[2]}, input range [{x.min():.3f}, {x.max():.3f}]")
    rows = []
    for n in range(1, 41):
        for r in RAISE_SCALES:
            try:
                ref.image_resize(torch.rand(1, n, 200), r)        # the short axis is H; 200 columns never raise at these scales
                raised = 0
            except Exception:
                raised = 1
            rows.append((n, r, raised))
    out["raise_table"] = np.array(rows, dtype=np.float64)
    print(f"raise table: {len(rows)} pairs, {int(sum(r[2] for r in rows))} raise")
    # _resize_matrix as it stands (the parent commit's values: the refactoring must not move a bit)
    mats = []
    for n, r, aa in MATRICES:
        m = imgproc._resize_matrix(n, math.ceil(n * r), r, aa)
        mats.append((n, r, int(aa), hashlib.sha256(m.tobytes()).hexdigest()))
    out["matrix_keys"] = np.array([(n, r, aa) for n, r, aa, _ in mats], dtype=np.float64)
    out["matrix_sha256"] = np.array([h for *_, h in mats])
    out["matrix_8_0375"] = imgproc._resize_matrix(8, 3, 0.375, True)
    out["matrix_4_05"] = imgproc._resize_matrix(4, 2, 0.5, True)
    path = os.path.join(HERE, "image_resize_native.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
