"""Helpers of tests/test_gpu_frames.py: the compact generator's case table (read from tests/test_gpu_compact.py, not copied) and
the float reference of the uint8 frame path -- what inference.py does per image."""
import numpy as np
import torch

from tests.test_gpu_compact import CASES, _model   # noqa: F401  (num_conv, upscale, act, batch, (h, w), channels_last, init)

PRECISIONS = ("fast", "exact16", "strict")

# output widths W*S = 4k+1, 4k+2, 4k+3 for S = 1 and S = 3; with n = 3, h = 3 no total pixel count is a multiple of 4
# (the byte-store tail of the 4-pixel groups): (upscale, w)
ODD_WIDTHS = [(1, 5), (1, 6), (1, 7), (3, 3), (3, 6), (3, 5)]


def random_frames(n, h, w, seed):
    """uint8 [n,h,w,3], uniformly random, the values 0 and 255 present."""
    u8 = np.random.RandomState(seed).randint(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    flat = u8.reshape(-1)
    flat[0], flat[-1] = 0, 255
    return u8


def float_reference(model, u8, channels_last=False):
    """The parent's path for every image of u8 [n,h,w,3]: astype(float32) / 255 -> image_to_tensor -> model -> tensor_to_image.
    Returns (uint8 [n,sH,sW,3], the fp32 model output)."""
    from real_esrgan_pytorch_amd import imgproc
    x = torch.stack([imgproc.image_to_tensor(f.astype(np.float32) / 255.0, False, False) for f in u8]).cuda()
    if channels_last:
        x = x.to(memory_format=torch.channels_last)
    with torch.no_grad():
        y = model(x)
    return np.stack([imgproc.tensor_to_image(y[i:i + 1], False, False) for i in range(y.shape[0])]), y
