"""real_esrgan-pytorch_amd -- the MI355X (gfx950) native Real-ESRGAN hot path.

Import as `real_esrgan_pytorch_amd` (the sibling shim package maps the importable name onto this
directory, whose name is fixed by the project layout and is not a valid Python identifier).

Contents: `model` (Generator / EMA behind the reference's nn.Module surface), `compact` (upstream's SRVGGNetCompact, forward only), `frames` (uint8 frames in, uint8 frames out: `upscale_u8`, `FrameStream`, `outscale`; YUV 4:2:0 frames: `upscale_yuv420`, 10-bit ones: `upscale_yuv420p10`; a source and a destination format of their own: `upscale_frames`, `FrameFormat`; grey, RGBA and 16-bit images: `upscale_image`), `jpeg_encode` (finished frames as JPEG files written on the device: `encode_jpeg`, `jpeg_files`), `png_encode` (finished images as lossless PNG files written on the device: `encode_png`, `png_files`), `device_data` (the training tiles resident in HBM: `DeviceTileSource`, config.data_source = "device"; LR / HR pairs of the user's own resident in HBM: `PairedDeviceSource`, config.data_source = "paired"; the training pair pool behind either: `PairPool`, config.pair_pool_size), `_lib` (ctypes
binding of csrc/libresr_hip.so, C-ABI in include/resr.h), `csrc/` (HIP kernels + the C-ABI).
"""
from . import _lib  # noqa: F401
from .model import EMA, Generator, ResidualDenseBlock, ResidualResidualDenseBlock, load_official_state_dict  # noqa: F401
from .compact import SRVGGNetCompact  # noqa: F401
from .discriminator import Discriminator  # noqa: F401
from .content_loss import ContentLoss  # noqa: F401
from . import frames  # noqa: F401
from .frames import FrameStream, from_u8, output_size, to_u8, upscale_u8  # noqa: F401
from .frames import rgb_to_yuv420, rgb_to_yuv420_np, upscale_yuv420, yuv420_tables, yuv420_to_rgb, yuv420_to_rgb_np  # noqa: F401
from .frames import (from_yuv420p10, rgb_to_yuv420p10_np, to_yuv420p10, upscale_yuv420p10, yuv420p10_tables,  # noqa: F401
                     yuv420p10_to_rgb_np)
from .frames import FrameFormat, PIXEL_FORMATS, YUV_MATRICES, upscale_frames  # noqa: F401
from .frames import from_image, grey_np, image_to_rgb_np, rgb_to_image_np, to_image, upscale_image  # noqa: F401
from . import jpeg_encode  # noqa: F401
from .jpeg_encode import encode_jpeg, jpeg_files  # noqa: F401
from . import png_encode  # noqa: F401
from .png_encode import encode_png, png_files, png_max_bytes  # noqa: F401

__all__ = ["EMA", "Generator", "SRVGGNetCompact", "Discriminator", "ContentLoss", "ResidualDenseBlock", "ResidualResidualDenseBlock",
           "load_official_state_dict", "frames", "FrameStream", "upscale_u8", "to_u8", "from_u8", "output_size",
           "yuv420_tables", "yuv420_to_rgb_np", "rgb_to_yuv420_np", "yuv420_to_rgb", "rgb_to_yuv420", "upscale_yuv420",
           "yuv420p10_tables", "yuv420p10_to_rgb_np", "rgb_to_yuv420p10_np", "from_yuv420p10", "to_yuv420p10", "upscale_yuv420p10",
           "FrameFormat", "PIXEL_FORMATS", "YUV_MATRICES", "upscale_frames",
           "image_to_rgb_np", "grey_np", "rgb_to_image_np", "from_image", "to_image", "upscale_image",
           "jpeg_encode", "encode_jpeg", "jpeg_files", "png_encode", "encode_png", "png_files", "png_max_bytes"]
