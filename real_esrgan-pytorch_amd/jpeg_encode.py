"""Finished frames leave the device as JPEG files (csrc/jpeg_encode.hip; resr_jpeg_encode of include/resr.h).

    buf, lengths = encode_jpeg(frames_u8, quality=95, subsampling="420")     # device tensors: uint8 [N, capacity], int64 [N]
    files = jpeg_files(frames_u8, quality=95)                                # list[bytes], one read-back

`frames_u8` is a uint8 [N,H,W,3] RGB tensor on the device (what `frames.upscale_u8` returns).  File i is `buf[i, :lengths[i]]`: a
complete baseline JFIF file (SOI .. EOI), byte for byte the definition of DESIGN "JPEG encode" (tests/jpeg_encode_ref.py is its numpy
form).  `capacity` (default: the raw frame, H * W * 3 bytes) is the room of one file; a frame whose file needs more gets
`lengths[i] = -(bytes it needs)` and nothing of its row is written -- `jpeg_files` raises for it and names the size.  Nothing here
synchronises: three launches on the current stream, the workspace and the header cached per geometry.

`restart_interval`: MCUs per restart segment (None: the library's default, `_lib.RESR_JPEG_DEFAULT_INTERVAL`); the segments are the
encoder's parallel units, so every file carries a DRI segment and RSTm markers.
"""
import functools
from typing import List, Optional, Tuple

import torch

from . import _lib

__all__ = ["encode_jpeg", "jpeg_files", "jpeg_max_bytes", "JPEG_SUBSAMPLINGS"]

JPEG_SUBSAMPLINGS = {"444": _lib.RESR_JPEG_444, "420": _lib.RESR_JPEG_420}


def _check_options(quality, subsampling, restart_interval, capacity, what: str) -> Tuple[int, int, int]:
    """ValueError for what the C entry would refuse, before the device is looked at -> (quality, subsampling constant, interval)."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"{what}: quality must be an int in 1..100, got {quality!r}")
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"{what}: subsampling must be one of {tuple(JPEG_SUBSAMPLINGS)}, got {subsampling!r}")
    if restart_interval is not None and (isinstance(restart_interval, bool) or not isinstance(restart_interval, int)
                                         or not 1 <= restart_interval <= 65535):
        raise ValueError(f"{what}: restart_interval must be None (the default, {_lib.RESR_JPEG_DEFAULT_INTERVAL}) or an int in 1..65535, "
                         f"got {restart_interval!r}")
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1):
        raise ValueError(f"{what}: capacity must be None (the raw frame's bytes) or an int >= 1, got {capacity!r}")
    return quality, JPEG_SUBSAMPLINGS[subsampling], restart_interval or 0


def _check_frames(frames, what: str) -> Tuple[int, int, int]:
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        got = f"{frames.dtype} {tuple(frames.shape)}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"{what}: expected a uint8 [N,H,W,3] tensor, got {got}")
    n, h, w = (int(v) for v in frames.shape[:3])
    if n < 1 or not 1 <= h <= 65535 or not 1 <= w <= 65535:
        raise ValueError(f"{what}: N must be at least 1 and H, W in 1..65535 (the SOF0 fields), got {tuple(frames.shape)}")
    return n, h, w


@functools.lru_cache(maxsize=None)
def _desc(n: int, h: int, w: int, subsampling: int, quality: int, interval: int):
    """(descriptor, header bytes, workspace bytes, max bytes) of a geometry: pure functions of it, host only."""
    d = _lib.JpegEncDesc(n, h, w, subsampling, quality, interval)
    host = (_lib.C.c_uint8 * _lib.RESR_JPEG_HEADER_BYTES)()
    got = _lib.lib().resr_jpeg_encode_header(_lib.C.byref(d), host, len(host))
    if got != len(host):
        _lib.check(got if got < 0 else -1, "resr_jpeg_encode_header")
    return d, bytes(host), int(_lib.lib().resr_jpeg_encode_workspace_bytes(_lib.C.byref(d))), int(_lib.lib().resr_jpeg_encode_max_bytes(_lib.C.byref(d)))


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


def jpeg_max_bytes(n_h_w: Tuple[int, int, int], quality: int = 95, subsampling: str = "420", restart_interval: Optional[int] = None) -> int:
    """The bound no file of this geometry exceeds (resr_jpeg_encode_max_bytes): a capacity of this size never overflows."""
    q, s, r = _check_options(quality, subsampling, restart_interval, None, "jpeg_max_bytes")
    n, h, w = n_h_w
    return _desc(int(n), int(h), int(w), s, q, r)[3]


def encode_jpeg(frames_u8: torch.Tensor, quality: int = 95, subsampling: str = "420", restart_interval: Optional[int] = None,
                capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 [N,H,W,3] on the device -> (buf uint8 [N, capacity], lengths int64 [N]), both on the device (module docstring)."""
    q, s, r = _check_options(quality, subsampling, restart_interval, capacity, "encode_jpeg")
    n, h, w = _check_frames(frames_u8, "encode_jpeg")
    _lib.require_cuda(frames_u8, "encode_jpeg")
    frames_u8 = frames_u8.contiguous()
    key = (n, h, w, s, q, r)
    d = _desc(*key)[0]
    header, workspace = _state(key, frames_u8.device)
    capacity = h * w * 3 if capacity is None else capacity
    buf = torch.empty((n, capacity), dtype=torch.uint8, device=frames_u8.device)
    lengths = torch.empty(n, dtype=torch.int64, device=frames_u8.device)
    _lib.check(_lib.lib().resr_jpeg_encode(_lib.C.byref(d), _lib.ptr(frames_u8), _lib.ptr(buf), capacity, _lib.ptr(lengths), _lib.ptr(header),
                                           header.numel(), _lib.ptr(workspace), workspace.numel() * 8, _lib.stream_ptr(frames_u8)),
               "resr_jpeg_encode")
    return buf, lengths


def jpeg_files(frames_u8: torch.Tensor, quality: int = 95, subsampling: str = "420", restart_interval: Optional[int] = None,
               capacity: Optional[int] = None) -> List[bytes]:
    """`encode_jpeg` and one read-back: the N files as bytes.  RuntimeError for a frame whose file did not fit `capacity`."""
    buf, lengths = encode_jpeg(frames_u8, quality, subsampling, restart_interval, capacity)
    sizes = lengths.cpu().tolist()
    for i, size in enumerate(sizes):
        if size < 0:
            raise RuntimeError(f"jpeg_files: the file of frame {i} needs {-size} bytes, the capacity is {buf.shape[1]}: pass capacity={-size} or more "
                               f"(jpeg_max_bytes gives a bound that always fits)")
    host = buf[:, :max(sizes)].cpu().numpy()
    return [host[i, :size].tobytes() for i, size in enumerate(sizes)]
