"""Finished images leave the device as PNG files, lossless (csrc/png_encode.hip; resr_png_encode of include/resr.h).

    buf, lengths = encode_png(images)          # device tensors: uint8 [N, capacity], int64 [N]
    files = png_files(images)                  # list[bytes], one read-back

`images` is a uint8 or uint16 [N,H,W,C] tensor on the device, C in 1, 3, 4 (grey, RGB, RGBA: what `frames.upscale_u8` and
`frames.upscale_image` return; a [N,H,W] tensor is grey).  File i is `buf[i, :lengths[i]]`: a complete PNG file that every reader accepts,
byte for byte the definition of DESIGN "PNG encode" (tests/png_encode_ref.py is its numpy form).  `capacity` (default: `png_max_bytes`,
about the raw image, which no file exceeds) is the room of one file; an image whose file needs more gets `lengths[i] = -(bytes it needs)`
and nothing of its row is written -- `png_files` raises for it and names the size.  Nothing here synchronises: four launches on the
current stream, the workspace and the header cached per geometry.

`segment_bytes`: bytes of the filtered stream per deflate block (None: the library's default, `_lib.RESR_PNG_DEFAULT_SEGMENT_BYTES`;
64..65535); the segments are the encoder's parallel units, one IDAT chunk each.
"""
import functools
from typing import List, Optional, Tuple

import torch

from . import _lib

__all__ = ["encode_png", "png_files", "png_max_bytes"]

_DEPTHS = {torch.uint8: 8, torch.uint16: 16, "uint8": 8, "uint16": 16}


def _check_options(segment_bytes, capacity, what: str) -> int:
    """ValueError for what the C entry would refuse, before the device is looked at -> segment_bytes as the descriptor takes it."""
    if segment_bytes is not None and (isinstance(segment_bytes, bool) or not isinstance(segment_bytes, int) or not 64 <= segment_bytes <= 65535):
        raise ValueError(f"{what}: segment_bytes must be None (the default, {_lib.RESR_PNG_DEFAULT_SEGMENT_BYTES}) or an int in 64..65535, "
                         f"got {segment_bytes!r}")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1):
        raise ValueError(f"{what}: capacity must be None (png_max_bytes of the geometry) or an int >= 1, got {capacity!r}")
    return segment_bytes or 0


def _check_shape(shape, dtype, what: str) -> Tuple[int, int, int, int, int]:
    """-> (n, h, w, channels, bit depth) of [N,H,W] or [N,H,W,C] images of a dtype (torch's, numpy's or its name)."""
    depth = _DEPTHS.get(dtype, _DEPTHS.get(str(getattr(dtype, "name", dtype))))
    shape = tuple(int(v) for v in shape)
    if depth is None or len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] not in (1, 3, 4)):
        raise ValueError(f"{what}: expected uint8 or uint16 [N,H,W,C] images with C in 1, 3, 4 (or [N,H,W]), got {dtype} {shape}")
    n, h, w = shape[:3]
    c = shape[3] if len(shape) == 4 else 1
    limit = (2 ** 31 - 1) // (c * depth // 8)
    if n < 1 or not 1 <= h <= limit or not 1 <= w <= limit:
        raise ValueError(f"{what}: N must be at least 1 and H, W in 1..{limit}, got {shape}")
    return n, h, w, c, depth


def _check_images(images, what: str) -> Tuple[int, int, int, int, int]:
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{what}: expected a uint8 or uint16 [N,H,W,C] tensor, got {type(images).__name__}")
    return _check_shape(images.shape, images.dtype, what)


@functools.lru_cache(maxsize=None)
def _desc(n: int, h: int, w: int, c: int, depth: int, segment_bytes: int):
    """(descriptor, header bytes, workspace bytes, max bytes) of a geometry: pure functions of it, host only."""
    d = _lib.PngEncDesc(n, h, w, c, depth, segment_bytes)
    host = (_lib.C.c_uint8 * _lib.RESR_PNG_HEADER_BYTES)()
    got = _lib.lib().resr_png_encode_header(_lib.C.byref(d), host, len(host))
    if got != len(host):
        _lib.check(got if got < 0 else -1, "resr_png_encode_header")
    ws_bytes, max_bytes = int(_lib.lib().resr_png_encode_workspace_bytes(_lib.C.byref(d))), int(_lib.lib().resr_png_encode_max_bytes(_lib.C.byref(d)))
    if not ws_bytes or not max_bytes:
        _lib.check(-1, "resr_png_encode_workspace_bytes")
    return d, bytes(host), ws_bytes, max_bytes


_device_state = {}      # (geometry key, device) -> (header on the device, workspace): reused by every call of that geometry on that device


def _state(key, device):
    st = _device_state.get((key, device))
    if st is None:
        _, header, ws_bytes, _ = _desc(*key)
        st = (torch.frombuffer(bytearray(header), dtype=torch.uint8).to(device), torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=device))
        if len(_device_state) >= 8:      # a stream of frames has one or two geometries: keep a few, not every size ever seen
            _device_state.pop(next(iter(_device_state)))
        _device_state[(key, device)] = st
    return st


def png_max_bytes(shape, dtype=torch.uint8, segment_bytes: Optional[int] = None) -> int:
    """The bound no file of [N,H,W,C] images of `dtype` exceeds (resr_png_encode_max_bytes): a capacity of this size never overflows."""
    s = _check_options(segment_bytes, None, "png_max_bytes")
    return _desc(*_check_shape(shape, dtype, "png_max_bytes"), s)[3]


def encode_png(images: torch.Tensor, segment_bytes: Optional[int] = None, capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 / uint16 [N,H,W,C] on the device -> (buf uint8 [N, capacity], lengths int64 [N]), both on the device (module docstring)."""
    s = _check_options(segment_bytes, capacity, "encode_png")
    key = _check_images(images, "encode_png") + (s,)
    _lib.require_cuda(images, "encode_png")
    images = images.contiguous()
    d, _, _, max_bytes = _desc(*key)
    header, workspace = _state(key, images.device)
    capacity = max_bytes if capacity is None else capacity
    buf = torch.empty((key[0], capacity), dtype=torch.uint8, device=images.device)
    lengths = torch.empty(key[0], dtype=torch.int64, device=images.device)
    _lib.check(_lib.lib().resr_png_encode(_lib.C.byref(d), _lib.ptr(images), _lib.ptr(buf), capacity, _lib.ptr(lengths), _lib.ptr(header),
                                          header.numel(), _lib.ptr(workspace), workspace.numel() * 8, _lib.stream_ptr(images)),
               "resr_png_encode")
    return buf, lengths


def png_files(images: torch.Tensor, segment_bytes: Optional[int] = None, capacity: Optional[int] = None) -> List[bytes]:
    """`encode_png` and one read-back: the N files as bytes.  RuntimeError for an image whose file did not fit `capacity`."""
    buf, lengths = encode_png(images, segment_bytes, capacity)
    sizes = lengths.cpu().tolist()
    for i, size in enumerate(sizes):
        if size < 0:
            raise RuntimeError(f"png_files: the file of image {i} needs {-size} bytes, the capacity is {buf.shape[1]}: pass capacity={-size} or more "
                               f"(png_max_bytes, the default, gives a bound that always fits)")
    host = buf[:, :max(sizes)].cpu().numpy()
    return [host[i, :size].tobytes() for i, size in enumerate(sizes)]
