"""Directory evaluation behind the reference's `test.py` (reference test.py:29-96): super-resolve every image of
`config.lr_dir` with the EMA weights of `config.model_path`, write the results to `config.sr_dir`, report the mean NIQE.
With `config.full_ref` = "torch" or "native" (RESR_FULL_REF) every result is also scored against the file of the same name in
`config.hr_dir`: the mean PSNR and SSIM of the Y channel -- or, with `config.full_ref_channels` = "rgb" (RESR_FULL_REF_CHANNELS),
BasicSR's RGB PSNR and channel-mean SSIM -- are printed after the NIQE line.

    RESR_MODE=test python -m real_esrgan_pytorch_amd.test

PIL does the file I/O (cv2 is absent from the image; the reference's BGR<->RGB swaps cancel out) and a local natural
sort replaces `natsort`.
"""
from __future__ import annotations

import os
import re
from typing import List

import torch

from . import _lib, config, imgproc
from .compact import SRVGGNetCompact
from .tiling import super_resolve


def natural_sorted(names: List[str]) -> List[str]:
    """`natsort.natsorted` for plain file names: digit runs compare as integers."""
    return sorted(names, key=lambda s: [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", s) if t])


def read_ground_truth(hr_dir: str, name: str, height: int, width: int) -> torch.Tensor:
    """The ground truth of `name` as a uint8 [1,H,W,3] host tensor; a missing file or one that is not height x width is an error naming it."""
    import numpy as np
    from PIL import Image
    path = os.path.join(hr_dir, name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"full-reference scoring: no ground truth `{path}` for `{name}`")
    with Image.open(path) as image:
        hr = np.array(image.convert("RGB"))
    if hr.shape[:2] != (height, width):
        raise ValueError(f"full-reference scoring: the ground truth `{path}` is {hr.shape[0]}x{hr.shape[1]}, the result for `{name}` {height}x{width}")
    return torch.from_numpy(hr)[None]


def main() -> float:
    torch.cuda.set_device(config.device)            # one process per GPU: every launch and side stream on this device
    from PIL import Image
    # config.g_arch: Generator or SRVGGNetCompact, at config.inference_precision -- the fp32 call site, test.py:79-80 (no autocast)
    model = config.build_generator(False)
    model = model.to(device=config.device, memory_format=torch.channels_last)              # test.py:32
    print("Build Real_ESRGAN model successfully.")
    checkpoint = torch.load(config.model_path, map_location=lambda storage, loc: storage, weights_only=False)
    current = model.state_dict()
    model.load_state_dict({k.replace("model.", ""): v for k, v in checkpoint["ema_state_dict"].items()
                           if k.replace("model.", "") in current})                         # test.py:36-40
    print(f"Load Real_ESRGAN model weights `{os.path.abspath(config.model_path)}` successfully.")
    os.makedirs(config.sr_dir, exist_ok=True)
    model.eval()
    niqe = config.build_niqe()
    full_ref = config.build_full_ref()
    scores = []                     # full_ref: (psnr, ssim) device tensors per file, read once at the end
    niqe_metrics = 0.0
    file_names = natural_sorted(os.listdir(config.lr_dir))
    total_files = len(file_names)
    for name in file_names:
        lr_image_path = os.path.join(config.lr_dir, name)
        print(f"Processing `{os.path.abspath(lr_image_path)}`...")
        lr_tensor = imgproc.image_to_tensor(imgproc.read_image_rgb(lr_image_path), False, False).unsqueeze_(0)
        lr_tensor = lr_tensor.to(device=config.device, memory_format=torch.channels_last, non_blocking=True)
        with torch.no_grad():
            sr_tensor = super_resolve(model, lr_tensor)                                    # test.py:79 (any frame size)
        if isinstance(model, SRVGGNetCompact):
            sr_tensor.clamp_(0, 1)      # the compact module does not clamp (Generator does, inside); upstream's inference does, NIQE quantises to 0..255
        Image.fromarray(imgproc.tensor_to_image(sr_tensor, False, False)).save(os.path.join(config.sr_dir, name))
        if full_ref is not None:
            hr = read_ground_truth(config.hr_dir, name, sr_tensor.shape[2], sr_tensor.shape[3])
            scores.append(torch.stack(full_ref(sr_tensor, hr.to(device=config.device, non_blocking=True))).reshape(2))
        niqe_metrics += niqe(sr_tensor).item()
    _lib.chain_health()             # fail loudly if a chained conv launch ever gave up on a neighbouring tile
    avg_niqe = 100 if niqe_metrics / total_files > 100 else niqe_metrics / total_files    # test.py:92
    print(f"NIQE: {avg_niqe:4.2f} 100u")
    if scores:
        avg_psnr, avg_ssim = torch.stack(scores).mean(dim=0).tolist()
        print(f"PSNR: {avg_psnr:4.2f} dB")
        print(f"SSIM: {avg_ssim:4.4f}")
    return avg_niqe


if __name__ == "__main__":
    main()
