"""The uint8 frame path: uint8 HWC images in, uint8 HWC images out (csrc/frames.hip).

The result of every function here is DEFINED as what the float path followed by `imgproc.tensor_to_image` produces, bit for
bit: a frame enters as `u8 / 255.0f`, runs through the model in the model's arithmetic, and leaves as `v * 255`, clamped to
[0, 255] and truncated (a NaN inside the net is outside that definition, as it is for `astype(uint8)`).

    from_u8(frames)            uint8 [N,H,W,3] -> fp32 [N,3,H,W]           one launch (resr_u8_to_nchw)
    to_u8(sr)                  fp32 [N,3,H,W]  -> uint8 [N,H,W,3]          one launch (resr_nchw_to_u8)
    upscale_u8(model, frames)  uint8 [N,H,W,3] -> uint8 [N,sH,sW,3]        any model, any frame size
    FrameStream(model, depth)  host ndarray in -> host ndarray out, `depth` frames in flight
    output_size(h, w, s, o)    the size of a frame upscaled with `outscale=o`: the one place that formula lives
    upscale_image(model, im)   grey, RGB or RGBA images of 8 or 16 bits -> the same mode, [N,sH,sW(,C)]  (IMAGE MODES below)
    PIXEL_FORMATS              one record per pixel format name (layout id, bits, packing, dtypes): the table `YUV_LAYOUTS`,
                               `YUV10_LAYOUTS` and `FrameStream.PIX_FMTS` are read from, and the 8- and 10-bit functions below share
                               their bodies through

`upscale_u8` is the one definition of the path: a model with a fused entry (`SRVGGNetCompact.forward_u8`) runs it when the frame
fits one call; every other case (the RRDB `Generator`, frames the tiler has to cut) is `to_u8(super_resolve(model, from_u8(f)))`.
There is no PyTorch fallback for the conversions: a missing kernel is an error of `_lib`.

OUTSCALE -- a final size that is not the network's factor (upstream's `-s / --outscale`).  For a model of factor `s`, an LR frame
`H x W` and `outscale = o` (a finite positive number, `o != s`; `None` or `o == s` is the path above, untouched):

    sr = model(x)                              fp32, not clamped: exactly the float path
    r = o / s                                  out_h = ceil(H * s * r), out_w = ceil(W * s * r)   (`output_size`)
    per axis a banded tap table                `imgproc.resize_band_tables`: idx [out, P] int32, w [out, P] float32,
                                               P = ceil(4 / min(r, 1)) + 2 -- the non-zero band of `imgproc._resize_matrix` (the
                                               reference's MATLAB-style `image_resize`: bicubic a = -0.5, antialiased when
                                               shrinking, symmetric edges), the reflection folded into idx, float32 arithmetic
    out = W-pass(H-pass(sr))                   each pass acc = fmaf(v[idx[k]], w[k], acc) from 0, k ascending, fp32 throughout
    u8 = trunc(clamp(out * 255.0f, 0, 255))    `imgproc.tensor_to_image`, as everywhere on this path

A model with a fused entry runs `resr_compact_forward_u8_scaled` (the full-size frame exists as LDS tiles only); every other case is
`super_resolve` -> `resr_image_resize` with uint8 output, the same device routine, hence the same bits.  A frame too small for the
reference's symmetric edge copy raises ValueError before any launch, as the reference's `image_resize` raises.

YUV 4:2:0 -- what video decoders deliver and encoders consume (NV12 from hardware, I420 / `yuv420p` from software): 1.5 bytes per
pixel instead of 3, which halves every byte count that bounds a stream.  A frame of luma size H x W (both even) is a uint8 array
[3H/2, W] (the usual numpy / OpenCV view; batches [N,3H/2,W], contiguous): `layout="i420"` is Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2];
`layout="nv12"` is Y [H,W], then [H/2,W/2,2] interleaved Cb,Cr.  The path is DEFINED as a composition over the RGB one, bit for bit:

    upscale_yuv420(model, f) == rgb_to_yuv420_np(upscale_u8(model, yuv420_to_rgb_np(f)))

and the two colour conversions are integer functions of bytes (studio range, BT.601 or BT.709, Q16 tables `yuv420_tables`, chroma
replicated on the way in and box-averaged unrounded on the way out): `yuv420_to_rgb_np` / `rgb_to_yuv420_np` below ARE the
definition; `yuv420_to_rgb` / `rgb_to_yuv420` are the same functions on the device, one launch each.  A model with a fused entry
(`SRVGGNetCompact.forward_yuv420`: both conversions inside the compact net's first and last kernel) runs it when the frame fits one
call, with `outscale` too (`resr_compact_forward_yuv420_scaled`: the resized tail of the RGB path with a YUV 4:2:0 output stage, one
launch sequence, no RGB frame); every other case (the RRDB `Generator`, tiled frames, a scale so small that no tile of even height and
width fits the resize kernel's LDS) is the composition of the device launches.

10-BIT YUV 4:2:0 -- what decoders deliver for most HEVC / AV1 material (P010 from hardware, `yuv420p10le` from software), and what an
encoder needs to keep 1024 levels of a smooth gradient instead of 256.  The geometry is the 8-bit one with a little-endian uint16 word
per sample: a frame is a uint16 array [3H/2, W] (batches [N,3H/2,W], contiguous; `torch.uint16` on the device), 3 bytes per pixel --
the rgb24 stream's byte count, not the 8-bit YUV stream's 1.5: this path buys precision and removes the host conversion, it does not
halve bytes again.  `layout="i420p10"` (rawvideo `yuv420p10le`): planes as "i420", the sample in the low 10 bits (read `word & 1023`,
written with the high 6 bits zero); `layout="p010"` (`p010le`): planes as "nv12", the sample in the high 10 bits (read `word >> 6`,
written `sample << 6`).  Every 16-bit word is legal input.  The conversions are the 8-bit ones with 64 / 512 / 1023 in place of
16 / 128 / 255 (`yuv420p10_tables`, `yuv420p10_to_rgb_np`, `rgb_to_yuv420p10_np`: these ARE the definition), a sample enters the
model as `rgb10 / 1023.0f` and leaves as q10(v) = trunc(clamp(v * 1023.0f, 0, 1023)), and the path is a composition, bit for bit:

    upscale_yuv420p10(model, f) == rgb_to_yuv420p10_np(q10(float_path(model, yuv420p10_to_rgb_np(f) / 1023.0f)))

with `float_path` the model's forward (or `tiling.super_resolve`) on fp32 NCHW, followed by `resize_with_plan` with `outscale`.  A model
with a fused entry (`SRVGGNetCompact.forward_yuv420p10`) runs it when the frame fits one call, with `outscale` too
(`resr_compact_forward_yuv420p10_scaled`): neither an RGB frame nor an fp32 copy of the input exists then, and the fp32 frames of the
float path exist as LDS tiles only.  Every other case is `to_yuv420p10(float_path(from_yuv420p10(f)))`, one launch each way, straight
between the frames and fp32.  Not provided: 12 / 16-bit samples (16 bits would overflow the int32 accumulators), full range,
4:2:2 / 4:4:4.

MIXED FRAME FORMATS -- a source and a destination format of their own: 8 bits in and 10 out (the 1024 levels of the network's fp32
output for an 8-bit source), BT.601 in and BT.709 out (SD material upscaled to HD), NV12 / P010 surfaces in and planar frames out, rgb24
on one side.  A frame format is a name of `PIXEL_FORMATS` plus, for the YUV names, a matrix (`FrameFormat`).  For a source `A` and a
destination `B`, with top = 255 or 1023 of a side:

    upscale_frames(model, f, A, B) == encode_B(q_B(float_path(decode_A(f) / top_A)))

`decode_A`: the identity on HWC bytes ("rgb24"), else `yuv420_to_rgb_np` / `yuv420p10_to_rgb_np` with A's layout and matrix; `/ top_A` one
fp32 IEEE division; `float_path` as above (with `outscale`: followed by `resize_with_plan`); q_B(v) = trunc(clamp(v * top_B, 0, top_B))
in fp32; `encode_B`: the identity, else `rgb_to_yuv420_np` / `rgb_to_yuv420p10_np` with B's layout and matrix.  For A == B this is, term
for term, what `upscale_u8`, `upscale_yuv420` and `upscale_yuv420p10` are defined as, and `upscale_frames` calls them.  YUV to YUV on a
model with the fused entry (`SRVGGNetCompact.forward_yuv420_mixed`: the head reads A, the tail recomputes the residual from A and writes
B) runs it when the frame fits one call -- with `outscale` where `resr_compact_yuv420_scaled_fits` finds an even tile for B's depth;
every other case (the RRDB `Generator`, tiled frames, "rgb24" on a side, a scale with no even tile) is the composition of the generic
launches above, the same functions on the same values, hence the same bits.

IMAGE MODES -- the still images upstream's `RealESRGANer.enhance` takes besides 8-bit RGB: grey, RGBA and 16 bits per channel
(transparent sprites, anime assets, 16-bit scans).  An image batch is uint8 (top = 255) or uint16 (top = 65535; `torch.uint16` on the
device): [N,H,W] or [N,H,W,1] grey, [N,H,W,3] RGB, [N,H,W,4] RGBA; planes = 2 for RGBA, else 1.  Three numpy functions ARE the definition:

    image_to_rgb_np(images) -> [planes*N,H,W,3]   RGB: itself; grey: the plane three times; RGBA: the N colour images, then the N alpha
                                                  planes, each three times (upstream's `alpha_upsampler="realesrgan"`: alpha goes through
                                                  the network as a grey image)
    grey_np(rgb)                                  (4899 R + 9617 G + 1868 B + 8192) >> 14 on integer levels, at both depths (cv2's
                                                  fixed-point RGB2GRAY: exact for R = G = B, within int32 at 65535)
    rgb_to_image_np(levels, channels)             RGB: itself; grey: `grey_np`; RGBA: the colour of the first N images, `grey_np` of the
                                                  last N as the fourth channel

    upscale_image(model, images) == rgb_to_image_np(q(float_path(image_to_rgb_np(images) / top)), channels)

`/ top` one fp32 IEEE division, `float_path` the model's fp32 forward on the planes * N images (residual included), q(v) = trunc(clamp(v *
top, 0, top)) in fp32: `imgproc.tensor_to_image`'s rule with top for 255.  (Upstream rounds, and takes grey of the float output; the
reference truncates, and so does this path, which takes grey of the quantised levels.)  uint8 RGB is `upscale_u8`.  A model with a fused
entry (`SRVGGNetCompact.forward_image`: the head reads the image's own words, the tail writes them) runs it when the planes * N images
fit one call; every other case (the RRDB `Generator`, tiled frames) is `to_image(super_resolve(model, from_image(images)))`, one launch
each way.  With `outscale` (OUTSCALE above: r = o / s, the banded tap tables, H pass then W pass in fp32) the float frames are resized
before they are quantised:

    upscale_image(model, images, outscale=o) == rgb_to_image_np(q(resize(float_path(image_to_rgb_np(images) / top), r)), channels)

so grey is taken of the three quantised, resized levels, and the RGBA alpha is the grey of the resized alpha images' levels.  The fused
entry (`forward_image(images, outscale=o)`, `resr_compact_forward_image_scaled`: neither the fp32 x4 frames of the planes * N network
images nor their resized fp32 frames exist on the device) runs under the rule above where `resr_compact_image_scaled_fits` finds a
tile; every other case is `to_image(resize_with_plan(super_resolve(model, from_image(images)), plan))`, the same device routines, hence
the same bits.  No `FrameStream` for these modes; `PIXEL_FORMATS` does not list them.
"""
from __future__ import annotations

import collections
import functools
import math
from typing import Deque, Iterable, Iterator, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib, tiling

__all__ = ["from_u8", "to_u8", "upscale_u8", "FrameStream", "output_size", "check_outscale", "yuv420_tables", "yuv420_to_rgb_np",
           "rgb_to_yuv420_np", "yuv420_to_rgb", "rgb_to_yuv420", "upscale_yuv420", "yuv420p10_tables", "yuv420p10_to_rgb_np",
           "rgb_to_yuv420p10_np", "from_yuv420p10", "to_yuv420p10", "upscale_yuv420p10", "PixelFormat", "PIXEL_FORMATS", "YUV_MATRICES",
           "FrameFormat", "frame_format", "upscale_frames", "image_to_rgb_np", "grey_np", "rgb_to_image_np", "from_image", "to_image",
           "upscale_image"]

class PixelFormat(NamedTuple):
    """One row of `PIXEL_FORMATS`: everything the frame path knows about a pixel format by name.  `layout`: ResrYuvDesc.layout of
    include/resr.h (None: "rgb24", HWC bytes, no descriptor); `bits` per sample; `semi_planar`: one interleaved CbCr plane instead of
    a Cb and a Cr plane; `high_bits`: the sample sits in the high bits of its 16-bit word ("p010")."""
    layout: Optional[int]
    bits: int
    semi_planar: bool
    high_bits: bool
    np_dtype: np.dtype
    torch_dtype: torch.dtype

    @property
    def top(self) -> int:
        """The highest level of a sample: 255 or 1023."""
        return (1 << self.bits) - 1


_U8, _U16 = (np.dtype(np.uint8), torch.uint8), (np.dtype(np.uint16), torch.uint16)
PIXEL_FORMATS = {"rgb24": PixelFormat(None, 8, False, False, *_U8),
                 "i420": PixelFormat(_lib.YUV_I420, 8, False, False, *_U8),
                 "nv12": PixelFormat(_lib.YUV_NV12, 8, True, False, *_U8),
                 "i420p10": PixelFormat(_lib.YUV_I420P10, 10, False, False, *_U16),
                 "p010": PixelFormat(_lib.YUV_P010, 10, True, True, *_U16)}
YUV_LAYOUTS = {name: f.layout for name, f in PIXEL_FORMATS.items() if f.layout is not None and f.bits == 8}
YUV10_LAYOUTS = {name: f.layout for name, f in PIXEL_FORMATS.items() if f.layout is not None and f.bits == 10}
_YUV_BY_BITS = {8: (YUV_LAYOUTS, *_U8), 10: (YUV10_LAYOUTS, *_U16)}            # per depth: its layout names, numpy and torch dtype
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}          # (Kr, Kb); Kg = 1 - Kr - Kb


class FrameFormat(NamedTuple):
    """What the frames of one side of `upscale_frames` are: a name of `PIXEL_FORMATS` and, for the YUV names, one of `YUV_MATRICES`
    ("rgb24" has none).  A plain `(pix_fmt, matrix)` pair is taken wherever a FrameFormat is; `frame_format` checks either."""
    pix_fmt: str
    matrix: Optional[str] = None

    @property
    def fmt(self) -> PixelFormat:
        return PIXEL_FORMATS[self.pix_fmt]


def frame_format(f, what: str) -> FrameFormat:
    """`f` (a FrameFormat, a `(pix_fmt, matrix)` pair, or the bare name "rgb24") as a checked FrameFormat; ValueError for a name that is
    not in PIXEL_FORMATS, a matrix that is not in YUV_MATRICES (a YUV name needs one) and a matrix given for "rgb24"."""
    if isinstance(f, str):
        f = (f,)
    if not isinstance(f, (tuple, list)) or not 1 <= len(f) <= 2:
        raise ValueError(f"{what}: a frame format is a FrameFormat or a (pix_fmt, matrix) pair, got {f!r}")
    f = FrameFormat(*f)
    if not isinstance(f.pix_fmt, str) or f.pix_fmt not in PIXEL_FORMATS:
        raise ValueError(f"{what}: pix_fmt must be one of {tuple(PIXEL_FORMATS)}, got {f.pix_fmt!r}")
    if f.fmt.layout is None:
        if f.matrix is not None:
            raise ValueError(f"{what}: rgb24 takes no matrix, got {f.matrix!r}")
    elif not isinstance(f.matrix, str) or f.matrix not in YUV_MATRICES:
        raise ValueError(f"{what}: the matrix of {f.pix_fmt!r} must be one of {sorted(YUV_MATRICES)}, got {f.matrix!r}")
    return f


def check_outscale(outscale, s: int, what: str) -> Optional[float]:
    """None when `outscale` asks for the network's own factor (None or == s), else the float; ValueError for anything that is not a
    finite positive number (a bool included)."""
    if outscale is None:
        return None
    if isinstance(outscale, bool) or not isinstance(outscale, (int, float)) or not math.isfinite(outscale) or outscale <= 0:
        raise ValueError(f"{what}: outscale must be a finite positive number, got {outscale!r}")
    return None if float(outscale) == float(s) else float(outscale)


def output_size(h: int, w: int, s: int, outscale=None) -> Tuple[int, int]:
    """(out_h, out_w) of an h x w frame through a model of factor s: (h * s, w * s), or with an outscale o != s the reference's
    `ceil(in * scale)` for in = h * s and scale r = o / s (Python float division)."""
    o = check_outscale(outscale, s, "output_size")
    if o is None:
        return h * s, w * s
    r = o / s
    return math.ceil(h * s * r), math.ceil(w * s * r)


def _check_frames(frames: torch.Tensor, what: str) -> None:
    _lib.require_cuda(frames, what)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or min(frames.shape) < 1:
        raise RuntimeError(f"{what}: expected a uint8 [N,H,W,3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise RuntimeError(f"{what}: frames must be contiguous (HWC bytes, as an image decoder leaves them)")


@torch.no_grad()
def from_u8(frames: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H,W,3] -> fp32 [N,3,H,W], every value `u8 / 255.0f` (numpy's `astype(float32) / 255.0`)."""
    _check_frames(frames, "from_u8")
    n, h, w, _ = frames.shape
    x = torch.empty((n, 3, h, w), dtype=torch.float32, device=frames.device)
    _lib.check(_lib.lib().resr_u8_to_nchw(_lib.ptr(frames), _lib.ptr(x), n, h, w, _lib.stream_ptr(frames)), "resr_u8_to_nchw")
    return x


@torch.no_grad()
def to_u8(sr: torch.Tensor) -> torch.Tensor:
    """fp32 [N,3,H,W] -> uint8 [N,H,W,3]: `* 255`, clamp to [0, 255], truncate -- `imgproc.tensor_to_image` per image."""
    _lib.require_cuda(sr, "to_u8")
    if sr.dtype != torch.float32 or sr.dim() != 4 or sr.shape[1] != 3 or min(sr.shape) < 1:
        raise RuntimeError(f"to_u8: expected an fp32 [N,3,H,W] tensor, got {sr.dtype} {tuple(sr.shape)}")
    if not sr.is_contiguous():
        sr = sr.contiguous()
    n, _, h, w = sr.shape
    y = torch.empty((n, h, w, 3), dtype=torch.uint8, device=sr.device)
    _lib.check(_lib.lib().resr_nchw_to_u8(_lib.ptr(sr), _lib.ptr(y), n, h, w, _lib.stream_ptr(sr)), "resr_nchw_to_u8")
    return y


def _resize_plan(h: int, w: int, s: int, o: Optional[float], device, plan=None):
    """The `imgproc.ResizePlan` of an h x w frame through a model of factor s at outscale o: `plan` when the caller holds one, else
    a new one (ValueError before any launch for a frame the rule refuses); None when o is."""
    if o is None or plan is not None:
        return plan
    from .imgproc import ResizePlan        # (function-local, as every use of imgproc on the frame path)
    return ResizePlan(h * s, w * s, o / s, device)


@torch.no_grad()
def upscale_u8(model, frames: torch.Tensor, halo: Optional[int] = None, outscale: Optional[float] = None, plan=None) -> torch.Tensor:
    """uint8 [N,H,W,3] on the model's device -> uint8 [N,sH,sW,3].  `halo`: the tiler's, for frames it has to cut
    (tiling.super_resolve; with halo >= model.receptive_radius the tiled result equals the whole-frame one).
    `outscale`: the final factor when it is not the model's (module docstring) -> uint8 [N, *output_size(H, W, s, outscale), 3];
    `plan`: a cached `imgproc.ResizePlan` of this frame size (FrameStream keeps one)."""
    _check_frames(frames, "upscale_u8")
    n, h, w, _ = frames.shape
    s = model.upscale_factor
    o = check_outscale(outscale, s, "upscale_u8")
    if o is None:
        if hasattr(model, "forward_u8") and tiling.fits_whole(model, n, h, w):
            return model.forward_u8(frames)
        return to_u8(tiling.super_resolve(model, from_u8(frames), halo))
    from .imgproc import resize_with_plan
    plan = _resize_plan(h, w, s, o, frames.device, plan)
    if hasattr(model, "forward_u8") and tiling.fits_whole(model, n, h, w):
        return model.forward_u8(frames, outscale=o, plan=plan)
    return resize_with_plan(tiling.super_resolve(model, from_u8(frames), halo), plan, u8=True)


# ---- YUV 4:2:0, 8 and 10 bits: one body each, the public names of a depth pick their rows of PIXEL_FORMATS ------------------------
def _check_matrix(matrix: str, what: str) -> None:
    if matrix not in YUV_MATRICES:
        raise ValueError(f"{what}: matrix must be one of {sorted(YUV_MATRICES)}, got {matrix!r}")


def _yuv_format(layout: str, matrix: str, what: str, bits: int) -> PixelFormat:
    """The row of a 4:2:0 layout of this depth; ValueError for any other name (the other depth's included) or an unknown matrix."""
    names = _YUV_BY_BITS[bits][0]
    if layout not in names:
        raise ValueError(f"{what}: layout must be one of {sorted(names)}, got {layout!r}")
    _check_matrix(matrix, what)
    return PIXEL_FORMATS[layout]


def _yuv_name(bits: int) -> str:
    """What the functions and C entries of a depth are called after."""
    return "yuv420" if bits == 8 else f"yuv420p{bits}"


def _tables(bits: int, matrix: str, quantised: bool, what: str) -> Tuple[np.ndarray, np.ndarray]:
    _check_matrix(matrix, what)
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    top, ys, cs = float((1 << bits) - 1), float(219 << (bits - 8)), float(112 << (bits - 8))      # 255, 219, 112 / 1023, 876, 448
    f = np.array([[ys * kr, ys * kg, ys * kb],
                  [-cs * kr / (1 - kb), -cs * kg / (1 - kb), cs],
                  [cs, -cs * kg / (1 - kr), -cs * kb / (1 - kr)]], dtype=np.float64) / top
    a, c = top / ys, top / (2 * cs)
    i = np.array([[a, 0.0, c * 2 * (1 - kr)],
                  [a, -c * 2 * (1 - kb) * kb / kg, -c * 2 * (1 - kr) * kr / kg],
                  [a, c * 2 * (1 - kb), 0.0]], dtype=np.float64)
    if not quantised:
        return f, i
    return np.rint(f * 65536).astype(np.int32), np.rint(i * 65536).astype(np.int32)


def yuv420_tables(matrix: str = "bt601", quantised: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """(FQ, IQ), int32 [3,3]: the Q16 tables of the studio-range conversions.  F (per uint8 level; rows Y, Cb, Cr over R, G, B) and
    I (rows R, G, B over Y - 16, Cb - 128, Cr - 128) are computed in float64 from the matrix' (Kr, Kb); FQ = rint(F * 65536),
    IQ = rint(I * 65536).  `quantised=False` returns the float64 (F, I) themselves (bt601: F * 255 and I / 255 are the tables the
    reference prints in `rgb2ycbcr` / `ycbcr2rgb`)."""
    return _tables(8, matrix, quantised, "yuv420_tables")


def yuv420p10_tables(matrix: str = "bt601", quantised: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """`yuv420_tables` for 10-bit samples: the same (Kr, Kb), the studio constants 876 / 448 / 1023 in place of 219 / 112 / 255
    (F per 10-bit level; I over Y - 64, Cb - 512, Cr - 512 with a = 1023 / 876, c = 1023 / 896).  (FQ, IQ) int32 [3,3], Q16, or
    with `quantised=False` the float64 (F, I)."""
    return _tables(10, matrix, quantised, "yuv420p10_tables")


def _yuv_hw(shape) -> Optional[Tuple[int, int]]:
    """THE RULE: (H, W) of the luma plane of a [..., 3H/2, W] array, H and W even; None for any other shape."""
    if len(shape) < 2 or shape[-2] < 3 or shape[-2] % 3 or shape[-1] < 2 or shape[-1] % 2:
        return None
    return shape[-2] // 3 * 2, shape[-1]


def _yuv_to_rgb_np(frames: np.ndarray, layout: str, matrix: str, what: str, bits: int) -> np.ndarray:
    fmt = _yuv_format(layout, matrix, what, bits)
    frames = np.asarray(frames)
    if frames.dtype != fmt.np_dtype:
        raise ValueError(f"{what}: expected {fmt.np_dtype}, got {frames.dtype}")
    hw = _yuv_hw(frames.shape)
    if hw is None:
        raise ValueError(f"{what}: a 4:2:0 frame is [3H/2, W] with H and W even (rows a multiple of 3), got {tuple(frames.shape)}")
    (h, w), lead = hw, frames.shape[:-2]
    v = frames.astype(np.int32)
    v = v >> 6 if fmt.high_bits else v & fmt.top
    y = v[..., :h, :] - (16 << (bits - 8))
    chroma = v[..., h:, :].reshape(lead + (-1,))
    if fmt.semi_planar:
        pairs = chroma.reshape(lead + (h // 2, w // 2, 2))
        cb, cr = pairs[..., 0], pairs[..., 1]
    else:
        planes = chroma.reshape(lead + (2, h // 2, w // 2))
        cb, cr = planes[..., 0, :, :], planes[..., 1, :, :]
    cb = np.repeat(np.repeat(cb - (128 << (bits - 8)), 2, axis=-2), 2, axis=-1)
    cr = np.repeat(np.repeat(cr - (128 << (bits - 8)), 2, axis=-2), 2, axis=-1)
    iq = _tables(bits, matrix, True, what)[1]
    rgb = np.stack([(int(iq[c, 0]) * y + int(iq[c, 1]) * cb + int(iq[c, 2]) * cr + 32768) >> 16 for c in range(3)], axis=-1)
    return np.clip(rgb, 0, fmt.top).astype(fmt.np_dtype)


def _rgb_to_yuv_np(rgb: np.ndarray, layout: str, matrix: str, what: str, bits: int) -> np.ndarray:
    fmt = _yuv_format(layout, matrix, what, bits)
    rgb = np.asarray(rgb)
    if rgb.dtype != fmt.np_dtype or rgb.ndim < 3 or rgb.shape[-1] != 3 or rgb.shape[-3] < 2 or rgb.shape[-3] % 2 or rgb.shape[-2] < 2 or rgb.shape[-2] % 2:
        raise ValueError(f"{what}: expected {fmt.np_dtype} [..., H, W, 3] with H and W even, got {rgb.dtype} {rgb.shape}")
    if bits > 8 and rgb.size and int(rgb.max()) > fmt.top:
        raise ValueError(f"{what}: a {bits}-bit level is at most {fmt.top}, got {int(rgb.max())}")
    lead, (h, w) = rgb.shape[:-3], rgb.shape[-3:-1]
    fq = _tables(bits, matrix, True, what)[0].astype(np.int32)
    v = rgb.astype(np.int32)
    y = ((v * fq[0]).sum(-1) + ((16 << (bits - 8)) << 16) + 32768) >> 16
    s = v.reshape(lead + (h // 2, 2, w // 2, 2, 3)).sum(axis=(-4, -2))
    cb = ((s * fq[1]).sum(-1) + ((128 << (bits - 8)) << 18) + (1 << 17)) >> 18
    cr = ((s * fq[2]).sum(-1) + ((128 << (bits - 8)) << 18) + (1 << 17)) >> 18
    chroma = np.stack([cb, cr], axis=-1) if fmt.semi_planar else np.stack([cb, cr], axis=-3)
    out = np.concatenate([y.reshape(lead + (h * w,)), chroma.reshape(lead + (h * w // 2,))], axis=-1)
    out = out << 6 if fmt.high_bits else out
    return out.reshape(lead + (h * 3 // 2, w)).astype(fmt.np_dtype)


def yuv420_to_rgb_np(frames: np.ndarray, layout: str = "i420", matrix: str = "bt601") -> np.ndarray:
    """THE DEFINITION (host, numpy): uint8 [..., 3H/2, W] -> uint8 [..., H, W, 3].  Pixel (y, x) takes Y[y,x], Cb[y//2,x//2],
    Cr[y//2,x//2]; rgb[c] = clamp((IQ[c] . (Y - 16, Cb - 128, Cr - 128) + 32768) >> 16, 0, 255), int32, >> = floor.  Every byte
    value is legal input."""
    return _yuv_to_rgb_np(frames, layout, matrix, "yuv420_to_rgb_np", 8)


def rgb_to_yuv420_np(rgb: np.ndarray, layout: str = "i420", matrix: str = "bt601") -> np.ndarray:
    """THE DEFINITION (host, numpy): uint8 [..., H, W, 3] (H, W even) -> uint8 [..., 3H/2, W].  Y = (FQ[0] . rgb + (16 << 16) +
    32768) >> 16 per pixel; Cb = (FQ[1] . S + (128 << 18) + (1 << 17)) >> 18 per 2x2 block, S the sum of its four (R, G, B), Cr
    likewise with FQ[2]: a centre-sited box average of the unrounded chroma.  No clamp is needed: over all RGB triples the
    outputs lie in Y 16..235, Cb / Cr 16..240."""
    return _rgb_to_yuv_np(rgb, layout, matrix, "rgb_to_yuv420_np", 8)


def yuv420p10_to_rgb_np(frames: np.ndarray, layout: str = "i420p10", matrix: str = "bt601") -> np.ndarray:
    """THE DEFINITION (host, numpy): uint16 [..., 3H/2, W] -> uint16 [..., H, W, 3], levels 0..1023.  A sample is `word & 1023`
    ("i420p10") or `word >> 6` ("p010"); pixel (y, x) takes Y[y,x], Cb[y//2,x//2], Cr[y//2,x//2]; rgb10[c] = clamp((IQ[c] . (Y - 64,
    Cb - 512, Cr - 512) + 32768) >> 16, 0, 1023), int32, >> = floor.  Every 16-bit word is legal input."""
    return _yuv_to_rgb_np(frames, layout, matrix, "yuv420p10_to_rgb_np", 10)


def rgb_to_yuv420p10_np(rgb: np.ndarray, layout: str = "i420p10", matrix: str = "bt601") -> np.ndarray:
    """THE DEFINITION (host, numpy): uint16 [..., H, W, 3] of levels 0..1023 (H, W even; a larger value is a ValueError) -> uint16
    [..., 3H/2, W].  Y = (FQ[0] . rgb10 + (64 << 16) + 32768) >> 16 per pixel; Cb = (FQ[1] . S + (512 << 18) + (1 << 17)) >> 18 per
    2x2 block, S the sum of its four (R, G, B), Cr likewise with FQ[2].  No clamp is needed: the outputs lie in Y 64..940, Cb / Cr
    64..960, and the largest accumulator is 251,789,200.  "i420p10" stores the sample (high 6 bits zero), "p010" `sample << 6`."""
    return _rgb_to_yuv_np(rgb, layout, matrix, "rgb_to_yuv420p10_np", 10)


@functools.lru_cache(maxsize=None)
def _desc(bits: int, layout: str, matrix: str) -> _lib.YuvDesc:
    what = "yuv_desc" if bits == 8 else "yuv10_desc"
    fmt = _yuv_format(layout, matrix, what, bits)
    fq, iq = _tables(bits, matrix, True, what)
    i9 = _lib.C.c_int32 * 9
    return _lib.YuvDesc(fmt.layout, i9(*[int(v) for v in fq.reshape(-1)]), i9(*[int(v) for v in iq.reshape(-1)]))


def yuv_desc(layout: str, matrix: str) -> _lib.YuvDesc:
    """The ResrYuvDesc of include/resr.h for these names (cached: the tables are a pure function of them)."""
    return _desc(8, layout, matrix)


def yuv10_desc(layout: str, matrix: str) -> _lib.YuvDesc:
    """`yuv_desc` for the 10-bit entries: a 10-bit layout and the tables of `yuv420p10_tables`."""
    return _desc(10, layout, matrix)


def _check_yuv(frames: torch.Tensor, what: str, bits: int) -> Tuple[int, int, int]:
    _, np_dtype, torch_dtype = _YUV_BY_BITS[bits]
    _lib.require_cuda(frames, what)
    hw = _yuv_hw(frames.shape) if frames.dtype == torch_dtype and frames.dim() == 3 and frames.shape[0] >= 1 else None
    if hw is None:
        raise RuntimeError(f"{what}: expected a {np_dtype} [N,3H/2,W] tensor with H and W even, got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise RuntimeError(f"{what}: frames must be contiguous (planes one after the other, as a video decoder leaves them)")
    return (frames.shape[0],) + hw


def check_yuv420(frames: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(n, H, W) of a uint8 [N,3H/2,W] device tensor; RuntimeError for anything else."""
    return _check_yuv(frames, what, 8)


def check_yuv420p10(frames: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(n, H, W) of a uint16 [N,3H/2,W] device tensor; RuntimeError for anything else."""
    return _check_yuv(frames, what, 10)


@torch.no_grad()
def yuv420_to_rgb(frames: torch.Tensor, layout: str = "i420", matrix: str = "bt601") -> torch.Tensor:
    """uint8 [N,3H/2,W] -> uint8 [N,H,W,3] on the device, one launch (resr_yuv420_to_rgb): `yuv420_to_rgb_np`, bit for bit."""
    desc = yuv_desc(layout, matrix)
    n, h, w = check_yuv420(frames, "yuv420_to_rgb")
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames.device)
    _lib.check(_lib.lib().resr_yuv420_to_rgb(_lib.ptr(frames), _lib.ptr(rgb), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(frames)),
               "resr_yuv420_to_rgb")
    return rgb


@torch.no_grad()
def rgb_to_yuv420(rgb: torch.Tensor, layout: str = "i420", matrix: str = "bt601") -> torch.Tensor:
    """uint8 [N,H,W,3] (H, W even) -> uint8 [N,3H/2,W] on the device, one launch (resr_rgb_to_yuv420): `rgb_to_yuv420_np`, bit for bit."""
    desc = yuv_desc(layout, matrix)
    _check_frames(rgb, "rgb_to_yuv420")
    n, h, w, _ = rgb.shape
    if h % 2 or w % 2:
        raise RuntimeError(f"rgb_to_yuv420: a 4:2:0 frame has an even height and width, got {h}x{w}")
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device=rgb.device)
    _lib.check(_lib.lib().resr_rgb_to_yuv420(_lib.ptr(rgb), _lib.ptr(out), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(rgb)),
               "resr_rgb_to_yuv420")
    return out


@torch.no_grad()
def from_yuv420p10(frames: torch.Tensor, layout: str = "i420p10", matrix: str = "bt601") -> torch.Tensor:
    """uint16 [N,3H/2,W] -> fp32 [N,3,H,W] on the device, one launch (resr_yuv420p10_to_nchw): `yuv420p10_to_rgb_np(f) / 1023.0f`
    as NCHW, bit for bit."""
    desc = yuv10_desc(layout, matrix)
    n, h, w = check_yuv420p10(frames, "from_yuv420p10")
    x = torch.empty((n, 3, h, w), dtype=torch.float32, device=frames.device)
    _lib.check(_lib.lib().resr_yuv420p10_to_nchw(_lib.ptr(frames), _lib.ptr(x), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(frames)),
               "resr_yuv420p10_to_nchw")
    return x


@torch.no_grad()
def to_yuv420p10(sr: torch.Tensor, layout: str = "i420p10", matrix: str = "bt601") -> torch.Tensor:
    """fp32 [N,3,H,W] (H, W even) -> uint16 [N,3H/2,W] on the device, one launch (resr_nchw_to_yuv420p10): `* 1023`, clamp to
    [0, 1023], truncate, then `rgb_to_yuv420p10_np`, bit for bit."""
    desc = yuv10_desc(layout, matrix)
    _lib.require_cuda(sr, "to_yuv420p10")
    if sr.dtype != torch.float32 or sr.dim() != 4 or sr.shape[1] != 3 or min(sr.shape) < 1:
        raise RuntimeError(f"to_yuv420p10: expected an fp32 [N,3,H,W] tensor, got {sr.dtype} {tuple(sr.shape)}")
    n, _, h, w = sr.shape
    if h % 2 or w % 2:
        raise RuntimeError(f"to_yuv420p10: a 4:2:0 frame has an even height and width, got {h}x{w}")
    if not sr.is_contiguous():
        sr = sr.contiguous()
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint16, device=sr.device)
    _lib.check(_lib.lib().resr_nchw_to_yuv420p10(_lib.ptr(sr), _lib.ptr(out), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(sr)),
               "resr_nchw_to_yuv420p10")
    return out


def yuv420_output_size(h: int, w: int, s: int, outscale, what: str) -> Tuple[int, int]:
    """`output_size`, which for a 4:2:0 result must be even both ways: ValueError otherwise (before any launch)."""
    out_h, out_w = output_size(h, w, s, outscale)
    if out_h % 2 or out_w % 2:
        raise ValueError(f"{what}: outscale={outscale!r} turns {h}x{w} into {out_h}x{out_w}; a 4:2:0 frame needs an even height and width")
    return out_h, out_w


def _upscale_yuv(model, frames: torch.Tensor, layout: str, matrix: str, outscale, plan, bits: int, compose) -> torch.Tensor:
    """What `upscale_yuv420` and `upscale_yuv420p10` share: the names, the geometry, `outscale` and the even-output rule, the plan, and
    the choice of the model's fused call -- with `outscale` only where the library finds a tile of even height and width within the
    resize kernel's LDS (`resr_compact_yuv420_scaled_fits`: no device work).  `compose(o, plan)`: the depth's own composition."""
    what = "upscale_" + _yuv_name(bits)
    _desc(bits, layout, matrix)
    n, h, w = _check_yuv(frames, what, bits)
    s = model.upscale_factor
    o = check_outscale(outscale, s, what)
    method = "forward_" + _yuv_name(bits)

    def fused() -> bool:
        return hasattr(model, method) and tiling.fits_whole(model, n, h, w)
    if o is None and fused():
        return getattr(model, method)(frames, layout, matrix)
    if o is not None:
        yuv420_output_size(h, w, s, o, what)
        plan = _resize_plan(h, w, s, o, frames.device, plan)              # ValueError before any launch, as in upscale_u8
        if fused() and _lib.lib().resr_compact_yuv420_scaled_fits(h, w, s, plan.out_h, plan.out_w, plan.taps_y, plan.taps_x, bits):
            return getattr(model, method)(frames, layout, matrix, outscale=o, plan=plan)
    return compose(o, plan)


@torch.no_grad()
def upscale_yuv420(model, frames: torch.Tensor, layout: str = "i420", matrix: str = "bt601", halo: Optional[int] = None,
                   outscale: Optional[float] = None, plan=None) -> torch.Tensor:
    """uint8 [N,3H/2,W] on the model's device -> uint8 [N,3sH/2,sW], same layout: bit for bit
    `rgb_to_yuv420_np(upscale_u8(model, yuv420_to_rgb_np(frames)))` (module docstring).  The one place that chooses between the
    fused call and the composition, as `upscale_u8` is for RGB; `halo`, `outscale` and `plan` are `upscale_u8`'s.  With `outscale`
    the result is [N, 3 out_h / 2, out_w] for `output_size(H, W, s, outscale)`; an odd out_h or out_w is a ValueError before any
    launch."""
    def compose(o, plan):
        rgb = upscale_u8(model, yuv420_to_rgb(frames, layout, matrix), halo, outscale=o, plan=plan)
        return rgb_to_yuv420(rgb, layout, matrix)
    return _upscale_yuv(model, frames, layout, matrix, outscale, plan, 8, compose)


@torch.no_grad()
def upscale_yuv420p10(model, frames: torch.Tensor, layout: str = "i420p10", matrix: str = "bt601", halo: Optional[int] = None,
                      outscale: Optional[float] = None, plan=None) -> torch.Tensor:
    """uint16 [N,3H/2,W] (10-bit 4:2:0) on the model's device -> uint16 [N,3sH/2,sW], same layout: the composition of the module
    docstring, bit for bit.  The one place that chooses between the fused call and the composition, as `upscale_yuv420` is for 8
    bits; `halo`, `outscale` and `plan` are `upscale_u8`'s.  With `outscale` the float frame is resized (`resize_with_plan`, fp32
    out) before it is quantised -- inside the fused call's last kernel, or as launches of its own where that call does not apply; an
    odd out_h or out_w is a ValueError before any launch."""
    def compose(o, plan):
        sr = tiling.super_resolve(model, from_yuv420p10(frames, layout, matrix), halo)
        if o is not None:
            from .imgproc import resize_with_plan
            sr = resize_with_plan(sr, plan)
        return to_yuv420p10(sr, layout, matrix)
    return _upscale_yuv(model, frames, layout, matrix, outscale, plan, 10, compose)


# ---- a source and a destination format of their own (module docstring, MIXED FRAME FORMATS) --------------------------------------
def format_desc(f: FrameFormat) -> _lib.YuvDesc:
    """The ResrYuvDesc of a checked YUV frame format."""
    return _desc(f.fmt.bits, f.pix_fmt, f.matrix)


def mixed_geometry(frames, a: FrameFormat, b: FrameFormat, s: int, o: Optional[float], what: str) -> Optional[Tuple[int, int, int, int]]:
    """(H, W, out_h, out_w) of `frames` in format `a` through a model of factor s (at outscale `o`) into format `b`, from the shape alone:
    ValueError for a YUV source that is not [N,3H/2,W] with H and W even, and for a YUV destination whose height or width comes out odd.
    None for a shape the device-side checks will refuse anyway."""
    shape = tuple(getattr(frames, "shape", ()))
    if a.fmt.layout is None:
        if len(shape) != 4 or shape[3] != 3 or min(shape) < 1:
            return None
        h, w = shape[1], shape[2]
    else:
        hw = _yuv_hw(shape) if len(shape) == 3 and shape[0] >= 1 else None
        if hw is None:
            raise ValueError(f"{what}: a {a.pix_fmt} frame batch is [N,3H/2,W] with H and W even (rows a multiple of 3), got {shape}")
        h, w = hw
    out_h, out_w = output_size(h, w, s, o) if b.fmt.layout is None else yuv420_output_size(h, w, s, o, what)
    return h, w, out_h, out_w


@torch.no_grad()
def upscale_frames(model, frames: torch.Tensor, src, dst=None, halo: Optional[int] = None, outscale: Optional[float] = None,
                   plan=None) -> torch.Tensor:
    """Frames in the format `src` on the model's device -> the upscaled frames in the format `dst` (None: `src`); each a `FrameFormat`
    or a `(pix_fmt, matrix)` pair: uint8 [N,H,W,3] for "rgb24", else [N,3H/2,W] uint8 ("i420", "nv12") or uint16 ("i420p10", "p010").
    Bit for bit `encode_dst(q_dst(float_path(decode_src(frames) / top_src)))` (module docstring, MIXED FRAME FORMATS).  The one place
    that chooses: the same format on both sides is `upscale_u8` / `upscale_yuv420` / `upscale_yuv420p10`; YUV to YUV on a model with
    `forward_yuv420_mixed`, a frame that fits one call and (with `outscale`) an even tile for the destination's depth is that fused
    call; everything else is the composition of the generic launches.  `halo`, `outscale`, `plan`: `upscale_u8`'s.  ValueError before
    the device is looked at: an unknown format or matrix, a matrix for "rgb24", an odd YUV source, an odd size of a YUV result."""
    what = "upscale_frames"
    a = frame_format(src, what)
    b = a if dst is None else frame_format(dst, what)
    s = model.upscale_factor
    o = check_outscale(outscale, s, what)
    geom = mixed_geometry(frames, a, b, s, o, what)
    if a == b:
        if a.fmt.layout is None:
            return upscale_u8(model, frames, halo, outscale=o, plan=plan)
        same = upscale_yuv420 if a.fmt.bits == 8 else upscale_yuv420p10
        return same(model, frames, a.pix_fmt, a.matrix, halo, outscale=o, plan=plan)
    if a.fmt.layout is None:
        _check_frames(frames, what)
        n = frames.shape[0]
    else:
        n = _check_yuv(frames, what, a.fmt.bits)[0]
    h, w = geom[:2]
    plan = _resize_plan(h, w, s, o, frames.device, plan)                      # ValueError before any launch, as in upscale_u8
    yuv_both = a.fmt.layout is not None and b.fmt.layout is not None
    if yuv_both and hasattr(model, "forward_yuv420_mixed") and tiling.fits_whole(model, n, h, w):
        if o is None or _lib.lib().resr_compact_yuv420_scaled_fits(h, w, s, plan.out_h, plan.out_w, plan.taps_y, plan.taps_x, b.fmt.bits):
            return model.forward_yuv420_mixed(frames, a, b, outscale=o, plan=plan)
    # the composition: the generic launch(es) of the way in, the float path, those of the way out
    if a.fmt.bits == 10:
        x = from_yuv420p10(frames, a.pix_fmt, a.matrix)
    else:
        x = from_u8(frames if a.fmt.layout is None else yuv420_to_rgb(frames, a.pix_fmt, a.matrix))
    sr = tiling.super_resolve(model, x, halo)
    if o is not None:
        from .imgproc import resize_with_plan
    if b.fmt.bits == 10:
        return to_yuv420p10(sr if o is None else resize_with_plan(sr, plan), b.pix_fmt, b.matrix)
    rgb = to_u8(sr) if o is None else resize_with_plan(sr, plan, u8=True)
    return rgb if b.fmt.layout is None else rgb_to_yuv420(rgb, b.pix_fmt, b.matrix)


# ---- image modes: grey, RGB and RGBA images of 8 or 16 bits (module docstring, IMAGE MODES) -------------------------------------
_IMAGE_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}
_GREY_R, _GREY_G, _GREY_B = 4899, 9617, 1868            # cv2's fixed-point RGB2GRAY, Q14: they sum to 2^14


def _image_geometry(shape, what: str, error=ValueError) -> Tuple[int, int, int, int]:
    """THE RULE: (N, H, W, channels) of an image batch -- [N,H,W] or [N,H,W,1] grey, [N,H,W,3] RGB, [N,H,W,4] RGBA."""
    shape = tuple(shape)
    if len(shape) == 3:
        shape += (1,)
    if len(shape) != 4 or shape[3] not in (1, 3, 4) or min(shape) < 1:
        raise error(f"{what}: an image batch is [N,H,W] or [N,H,W,1] (grey), [N,H,W,3] (RGB) or [N,H,W,4] (RGBA), got {tuple(shape)}")
    return shape


def _image_np(images, what: str) -> Tuple[np.ndarray, int]:
    """`images` as a [N,H,W,C] array of uint8 or uint16, and C."""
    images = np.asarray(images)
    if images.dtype not in _IMAGE_DTYPES:
        raise ValueError(f"{what}: expected uint8 or uint16, got {images.dtype}")
    n, h, w, c = _image_geometry(images.shape, what)
    return images.reshape(n, h, w, c), c


def image_to_rgb_np(images: np.ndarray) -> np.ndarray:
    """THE DEFINITION (host, numpy): an image batch -> the RGB images the network runs on, [planes * N, H, W, 3] of the same dtype.
    RGB: the images themselves; grey: the plane three times; RGBA: the N colour images, then the N alpha planes, each three times
    (upstream's `alpha_upsampler="realesrgan"`: alpha goes through the network as a grey image)."""
    images, c = _image_np(images, "image_to_rgb_np")
    if c == 3:
        return images
    if c == 1:
        return np.repeat(images, 3, axis=3)
    return np.concatenate([images[..., :3], np.repeat(images[..., 3:], 3, axis=3)], axis=0)


def grey_np(rgb: np.ndarray) -> np.ndarray:
    """THE DEFINITION (host, numpy): uint8 or uint16 [..., 3] -> [...] of the same dtype, `(4899 R + 9617 G + 1868 B + 8192) >> 14`
    on integer levels at both depths -- cv2's fixed-point RGB2GRAY.  The coefficients sum to 2^14, so a grey triple (v, v, v) gives v
    exactly, and the sum stays below 2^31 at 65535.  Within 1 level of rint(0.299 R + 0.587 G + 0.114 B) at 8 bits, 2 at 16."""
    rgb = np.asarray(rgb)
    if rgb.dtype not in _IMAGE_DTYPES or rgb.ndim < 1 or rgb.shape[-1] != 3:
        raise ValueError(f"grey_np: expected uint8 or uint16 [..., 3], got {rgb.dtype} {rgb.shape}")
    v = rgb.astype(np.int64)
    return ((_GREY_R * v[..., 0] + _GREY_G * v[..., 1] + _GREY_B * v[..., 2] + 8192) >> 14).astype(rgb.dtype)


def rgb_to_image_np(rgb_levels: np.ndarray, channels: int) -> np.ndarray:
    """THE DEFINITION (host, numpy): the quantised network output [planes * N, H, W, 3] -> the image batch.  channels = 3: itself;
    1: `grey_np` -> [N,H,W]; 4: the colour of the first N images and `grey_np` of the last N as the fourth channel -> [N,H,W,4]."""
    rgb = np.asarray(rgb_levels)
    if rgb.dtype not in _IMAGE_DTYPES or rgb.ndim != 4 or rgb.shape[3] != 3:
        raise ValueError(f"rgb_to_image_np: expected uint8 or uint16 [planes * N, H, W, 3], got {rgb.dtype} {rgb.shape}")
    if channels == 3:
        return rgb
    if channels == 1:
        return grey_np(rgb)
    if channels != 4:
        raise ValueError(f"rgb_to_image_np: channels must be 1, 3 or 4, got {channels!r}")
    if rgb.shape[0] % 2:
        raise ValueError(f"rgb_to_image_np: an RGBA batch is N colour images and N alpha images, got {rgb.shape[0]} images")
    n = rgb.shape[0] // 2
    return np.concatenate([rgb[:n], grey_np(rgb[n:])[..., None]], axis=3)


def check_images(images: torch.Tensor, what: str) -> Tuple[int, int, int, int]:
    """(N, H, W, channels) of a contiguous uint8 / uint16 image batch on the device; RuntimeError for anything else, before any launch."""
    _lib.require_cuda(images, what)
    if images.dtype not in _IMAGE_DTYPES.values():
        raise RuntimeError(f"{what}: expected a uint8 or uint16 image batch, got {images.dtype} {tuple(images.shape)}")
    geom = _image_geometry(images.shape, what, RuntimeError)
    if not images.is_contiguous():
        raise RuntimeError(f"{what}: images must be contiguous (HWC words, as an image decoder leaves them)")
    return geom


def image_desc(channels: int, dtype) -> _lib.ImageDesc:
    """The ResrImageDesc of include/resr.h: channels 1, 3 or 4; 8 bits for torch.uint8, 16 for torch.uint16."""
    if channels not in (1, 3, 4) or dtype not in _IMAGE_DTYPES.values():
        raise ValueError(f"image_desc: channels 1, 3 or 4 of torch.uint8 or torch.uint16, got {channels!r} of {dtype!r}")
    return _lib.ImageDesc(channels, 8 if dtype == torch.uint8 else 16)


@torch.no_grad()
def from_image(images: torch.Tensor) -> torch.Tensor:
    """An image batch on the device -> fp32 [planes * N, 3, H, W], one launch (resr_image_to_nchw): `image_to_rgb_np(images) / top` as
    NCHW, bit for bit (top = 255 or 65535, one IEEE division)."""
    n, h, w, c = check_images(images, "from_image")
    desc = image_desc(c, images.dtype)
    x = torch.empty(((2 if c == 4 else 1) * n, 3, h, w), dtype=torch.float32, device=images.device)
    _lib.check(_lib.lib().resr_image_to_nchw(_lib.ptr(images), _lib.ptr(x), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(images)),
               "resr_image_to_nchw")
    return x


@torch.no_grad()
def to_image(sr: torch.Tensor, channels: int, dtype) -> torch.Tensor:
    """fp32 [planes * N, 3, H, W] -> the image batch [N,H,W,channels] of `dtype` (grey: [N,H,W]), one launch (resr_nchw_to_image):
    `* top`, clamp to [0, top], truncate, then `rgb_to_image_np`, bit for bit."""
    desc = image_desc(channels, dtype)
    _lib.require_cuda(sr, "to_image")
    planes = 2 if channels == 4 else 1
    if sr.dtype != torch.float32 or sr.dim() != 4 or sr.shape[1] != 3 or min(sr.shape) < 1 or sr.shape[0] % planes:
        raise RuntimeError(f"to_image: expected an fp32 [{'2N' if planes == 2 else 'N'},3,H,W] tensor, got {sr.dtype} {tuple(sr.shape)}")
    if not sr.is_contiguous():
        sr = sr.contiguous()
    n, _, h, w = sr.shape
    n //= planes
    y = torch.empty((n, h, w) if channels == 1 else (n, h, w, channels), dtype=dtype, device=sr.device)
    _lib.check(_lib.lib().resr_nchw_to_image(_lib.ptr(sr), _lib.ptr(y), n, h, w, _lib.C.byref(desc), _lib.stream_ptr(sr)), "resr_nchw_to_image")
    return y


@torch.no_grad()
def upscale_image(model, images: torch.Tensor, halo: Optional[int] = None, outscale: Optional[float] = None, plan=None) -> torch.Tensor:
    """An image batch on the model's device -- uint8 or uint16, [N,H,W] or [N,H,W,1] grey, [N,H,W,3] RGB, [N,H,W,4] RGBA, contiguous
    -> the upscaled batch of the same dtype and trailing shape, [N,sH,sW(,C)].  Bit for bit
    `rgb_to_image_np(q(float_path(image_to_rgb_np(images) / top)), channels)` (module docstring, IMAGE MODES).  The one place that
    chooses, by `upscale_u8`'s rule: uint8 RGB IS `upscale_u8`; a model with the fused entry (`SRVGGNetCompact.forward_image`) runs it
    when the network's batch of planes * N images fits one call; every other case (the RRDB `Generator`, frames the tiler has to cut)
    is `to_image(super_resolve(model, from_image(images)))`.  `halo`: `upscale_u8`'s.

    `outscale`, `plan`: `upscale_u8`'s -> [N, *output_size(H, W, s, outscale)(, C)]: the float frames are resized (`resize_with_plan`,
    fp32 out) before they are quantised -- inside the fused call's last kernel where the library finds a tile within the resize kernel's
    LDS (`resr_compact_image_scaled_fits`: no device work), else as a launch of its own between `super_resolve` and `to_image`.  A bad
    outscale and a frame the resize rule refuses are ValueErrors before any launch."""
    n, h, w, c = check_images(images, "upscale_image")
    s = model.upscale_factor
    o = check_outscale(outscale, s, "upscale_image")
    if c == 3 and images.dtype == torch.uint8:
        return upscale_u8(model, images, halo, outscale=o, plan=plan)
    planes = 2 if c == 4 else 1
    fused = hasattr(model, "forward_image") and tiling.fits_whole(model, planes * n, h, w)
    if o is None:
        out_h, out_w = h * s, w * s
        if fused:
            out = model.forward_image(images)
        else:
            out = to_image(tiling.super_resolve(model, from_image(images), halo), c, images.dtype)
    else:
        plan = _resize_plan(h, w, s, o, images.device, plan)                  # ValueError before any launch, as in upscale_u8
        out_h, out_w = plan.out_h, plan.out_w
        bits = 8 if images.dtype == torch.uint8 else 16
        if fused and _lib.lib().resr_compact_image_scaled_fits(h, w, s, out_h, out_w, plan.taps_y, plan.taps_x, c, bits):
            out = model.forward_image(images, outscale=o, plan=plan)
        else:
            from .imgproc import resize_with_plan
            out = to_image(resize_with_plan(tiling.super_resolve(model, from_image(images), halo), plan), c, images.dtype)
    return out.reshape((n, out_h, out_w) + tuple(images.shape[3:]))


class _Slot:
    """One frame in flight: pinned host buffers, the device input, the events that order its three stages."""

    def __init__(self, in_shape: Tuple[int, ...], out_shape: Tuple[int, ...], device, dtype=torch.uint8, out_dtype=None) -> None:
        self.pin_in = torch.empty((1,) + in_shape, dtype=dtype, pin_memory=True)
        self.pin_out = torch.empty((1,) + out_shape, dtype=out_dtype or dtype, pin_memory=True)
        self.np_in, self.np_out = self.pin_in.numpy()[0], self.pin_out.numpy()[0]
        self.dev_in = torch.empty((1,) + in_shape, dtype=dtype, device=device)
        self.dev_out: Optional[torch.Tensor] = None      # held until the slot's next submit: its download has been waited for by then
        self.uploaded, self.computed, self.downloaded = (torch.cuda.Event() for _ in range(3))
        self.used = False
        # FrameStream.jpeg / .png: the file and its length on the device (held like dev_out), the length's pinned twin, the event behind the encode
        self.jpeg_buf = self.jpeg_len = self.pin_len = self.encoded = None


class FrameStream:
    """Pipelined host-to-host frames: `depth` slots, each a pinned uint8 input buffer, a pinned uint8 output buffer and their
    device twins; an upload stream, the compute stream (the current stream at the first submit) and a download stream, ordered
    by events only.  The host waits for one thing: the download event of the frame it hands back.

        with FrameStream(model, depth=2) as fs:
            for sr in fs.map(frames):          # HxWx3 uint8 ndarrays in, (sH)x(sW)x3 uint8 ndarrays out, input order
                ...

    `submit(frame)` enqueues a frame (at most `depth` may be pending), `result()` returns the oldest pending one.  With
    `copy=True` (default) the returned array is the caller's own; with `copy=False` it is a view of the slot's pinned buffer,
    valid until that slot is submitted to again, i.e. for `depth - 1` further submits (the `depth`-th overwrites it).  A frame of
    another size drains the pipeline (pending results are kept, in order) and reallocates.  No graph capture here.

    `outscale` (module docstring): results are `output_size(H, W, s, outscale)` frames; the slots are sized by it and the tap
    tables of the frame size are built once, kept with the slots and dropped with them on a change of size.

    `pix_fmt`: "rgb24" (default: everything above) or a YUV 4:2:0 layout, "i420" / "nv12" (module docstring), with `matrix`
    "bt601" / "bt709": `submit` takes a [3H/2, W] uint8 ndarray and `result` returns [3 out_h / 2, out_w]; each frame is
    `upscale_yuv420` of it, the slots are half the bytes, everything else is as above.  "i420p10" / "p010" (10-bit 4:2:0, module
    docstring): the same with uint16 ndarrays, each frame `upscale_yuv420p10` of it, the slots 3 bytes per pixel as for rgb24.

    `out_pix_fmt`, `out_matrix`: the format of the results when it is not the input's (None, the default: the input's) -- "nv12" in
    and "p010" out, "bt601" in and "bt709" out, "rgb24" on one side (then `out_matrix` stays None); each frame is `upscale_frames` of
    it (module docstring, MIXED FRAME FORMATS) and the output slots get the result's dtype and shape (`slot_layout`).

    `on_device` (attribute, default None): a callable given every result as the device tensor the last kernel wrote ([1, ...] of
    the output format), on the compute stream, right behind the frame's launches and before its download -- a quality score taken
    from the frame where it lies (`inference_frames --niqe`).  What it returns is dropped; it must not keep the tensor.

    `jpeg` (attribute, like `on_device`; None, the default: everything above): set it to `dict(quality=95, subsampling="420",
    restart_interval=None)`, any key optional, before the first submit or while no result is outstanding (else RuntimeError) --
    rgb24 results only (on a stream with a YUV `pix_fmt` / `out_pix_fmt` it is a ValueError, as are options `encode_jpeg` would
    refuse).  It is an attribute and not a constructor argument because the constructor's parameter list is pinned by the mixed-format
    surface test.  Every result is then the frame's JPEG FILE, a 1-D
    uint8 array: `jpeg_encode.encode_jpeg` of the frame on the compute stream, behind `on_device` (which still sees the raw frame),
    with the raw frame's size as capacity.  Only the file's bytes and its length cross the bus: the length (8 bytes) is downloaded
    behind the encode, `result()` waits for it and then downloads exactly that many bytes into the slot's pinned buffer (which keeps
    the raw frame's size).  A file that does not fit the capacity (`jpeg_capacity`, None: the raw frame's bytes) is not written by
    the device: that frame is downloaded raw and encoded by Pillow on the host with the same quality and subsampling, and counted in
    `jpeg_fallbacks`.

    `png` (attribute, the lossless twin of `jpeg`; None, the default: everything above): set it to `dict(segment_bytes=None)`, the key
    optional, under the same rules -- rgb24 results only, no result outstanding, and not together with `jpeg` (ValueError, whichever is
    set second).  Every result is then the frame's PNG FILE, a 1-D uint8 array: `png_encode.encode_png` of the frame on the compute
    stream, behind `on_device`, downloaded length first and then exactly its bytes.  The capacity is the raw frame's bytes, the size of the
    slot's pinned buffer (`png_capacity`, None: that; a smaller value lowers it): a picture's file is below it, noise's is not.  A file that
    does not fit is not written by the device: that frame is downloaded raw and saved by Pillow as PNG, and counted in `png_fallbacks`."""

    PIX_FMTS = tuple(PIXEL_FORMATS)

    def __init__(self, model, depth: int = 2, outscale: Optional[float] = None, pix_fmt: str = "rgb24", matrix: str = "bt601",
                 out_pix_fmt: Optional[str] = None, out_matrix: Optional[str] = None) -> None:
        if isinstance(depth, bool) or not isinstance(depth, int) or depth < 1:
            raise ValueError(f"FrameStream: depth must be an int >= 1, got {depth!r}")
        if pix_fmt not in self.PIX_FMTS:
            raise ValueError(f"FrameStream: pix_fmt must be one of {self.PIX_FMTS}, got {pix_fmt!r}")
        _check_matrix(matrix, "FrameStream")
        self.pix_fmt, self.matrix = pix_fmt, matrix
        # what is not given is the input's; a result in rgb24 has no matrix, and one given for it is refused
        self.out_pix_fmt = pix_fmt if out_pix_fmt is None else out_pix_fmt
        self.out_matrix = out_matrix if out_matrix is not None or self.out_pix_fmt == "rgb24" else matrix
        frame_format((self.out_pix_fmt, self.out_matrix), "FrameStream")
        self._fmt = _StreamFormat(pix_fmt, matrix, self.out_pix_fmt, self.out_matrix)
        self._jpeg, self.jpeg_capacity, self.jpeg_fallbacks = None, None, 0
        self._png, self.png_capacity, self.png_fallbacks = None, None, 0
        self.outscale = check_outscale(outscale, getattr(model, "upscale_factor", 0), "FrameStream")
        self._plan = None
        param = next(iter(model.parameters()), None)
        if param is None or not param.is_cuda:
            raise RuntimeError("FrameStream: the model must be on the MI355X device (model.cuda()); this package has no CPU path")
        self.model, self.depth, self.device = model, depth, param.device
        self._slots: List[_Slot] = []
        self._shape = None
        self._next = 0
        self._pending: Deque[_Slot] = collections.deque()
        self._ready: Deque[np.ndarray] = collections.deque()     # results drained by a change of frame size
        self._up = self._down = self._compute = None
        self._closed = False
        self.on_device = None

    @property
    def jpeg(self) -> Optional[dict]:
        """None, or the options every result is encoded with (class docstring): quality, subsampling, restart_interval."""
        return self._jpeg

    @jpeg.setter
    def jpeg(self, options: Optional[dict]) -> None:
        if options is not None:
            from . import jpeg_encode
            if not isinstance(options, dict) or set(options) - {"quality", "subsampling", "restart_interval"}:
                raise ValueError(f"FrameStream: jpeg must be None or a dict with keys among quality, subsampling, restart_interval, got {options!r}")
            if self.pix_fmt != "rgb24" or self.out_pix_fmt != "rgb24":
                raise ValueError(f"FrameStream: jpeg needs rgb24 frames on both sides, got pix_fmt={self.pix_fmt!r}, out_pix_fmt={self.out_pix_fmt!r} "
                                 "(encoding from the YUV formats is not built)")
            options = dict(quality=options.get("quality", 95), subsampling=options.get("subsampling", "420"), restart_interval=options.get("restart_interval"))
            jpeg_encode._check_options(options["quality"], options["subsampling"], options["restart_interval"], None, "FrameStream")
            if self._png is not None:
                raise ValueError("FrameStream: jpeg and png cannot both be set: a result is one file (set png to None first)")
        if len(self):
            raise RuntimeError(f"FrameStream: {len(self)} results are outstanding; take them before jpeg is changed (they were submitted under the old setting)")
        self._jpeg = options

    @property
    def png(self) -> Optional[dict]:
        """None, or the options every result is encoded with as a PNG file (class docstring): segment_bytes."""
        return self._png

    @png.setter
    def png(self, options: Optional[dict]) -> None:
        if options is not None:
            from . import png_encode
            if not isinstance(options, dict) or set(options) - {"segment_bytes"}:
                raise ValueError(f"FrameStream: png must be None or a dict with no key but segment_bytes, got {options!r}")
            if self.pix_fmt != "rgb24" or self.out_pix_fmt != "rgb24":
                raise ValueError(f"FrameStream: png needs rgb24 frames on both sides, got pix_fmt={self.pix_fmt!r}, out_pix_fmt={self.out_pix_fmt!r} "
                                 "(the YUV formats have no PNG colour type)")
            options = dict(segment_bytes=options.get("segment_bytes"))
            png_encode._check_options(options["segment_bytes"], None, "FrameStream")
            if self._jpeg is not None:
                raise ValueError("FrameStream: jpeg and png cannot both be set: a result is one file (set jpeg to None first)")
        if len(self):
            raise RuntimeError(f"FrameStream: {len(self)} results are outstanding; take them before png is changed (they were submitted under the old setting)")
        self._png = options

    @staticmethod
    def check_frame(frame) -> None:
        _check_host_frame(frame, PIXEL_FORMATS["rgb24"])

    @staticmethod
    def check_frame_yuv420(frame) -> None:
        _check_host_frame(frame, PIXEL_FORMATS["i420"])

    @staticmethod
    def check_frame_yuv420p10(frame) -> None:
        _check_host_frame(frame, PIXEL_FORMATS["i420p10"])

    def slot_layout(self, h: int, w: int):
        """((in_shape, in_dtype), (out_shape, out_dtype)) of the slots of an h x w frame, numpy dtypes: what `submit` takes and
        `result` returns.  No device work; ValueError for a result the output format cannot hold (an odd 4:2:0 size)."""
        in_shape, out_shape = self._fmt.shapes(h, w, self.model.upscale_factor, self.outscale)
        return (in_shape, self._fmt.fmt.np_dtype), (out_shape, self._fmt.out_fmt.np_dtype)

    def __len__(self) -> int:
        """Results not yet taken."""
        return len(self._ready) + len(self._pending)

    def _drain(self) -> None:
        while self._pending:
            self._ready.append(self._take(self._pending.popleft(), True))

    def _take(self, slot: _Slot, copy: bool) -> np.ndarray:
        slot.downloaded.synchronize()
        _lib.chain_health()          # every launch of this frame has reported: a broken chained launch must not reach the caller
        if self.jpeg is not None or self.png is not None:
            return self._take_jpeg(slot, copy)
        return slot.np_out.copy() if copy else slot.np_out

    def _take_jpeg(self, slot: _Slot, copy: bool) -> np.ndarray:
        """The file of a slot whose length has arrived (`downloaded`): its bytes, or on overflow the raw frame and Pillow."""
        size = int(slot.pin_len[0])
        flat = slot.pin_out.view(-1)
        with torch.cuda.stream(self._down):      # (the download stream is behind the encode already: it carried the length)
            if size >= 0:
                flat[:size].copy_(slot.jpeg_buf[0, :size], non_blocking=True)
            else:
                slot.pin_out.copy_(slot.dev_out, non_blocking=True)
            slot.downloaded.record(self._down)
        slot.downloaded.synchronize()
        if size >= 0:
            data = flat.numpy()[:size]
            return data.copy() if copy else data
        import io
        from PIL import Image
        file = io.BytesIO()
        if self.png is not None:
            self.png_fallbacks += 1
            Image.fromarray(slot.np_out).save(file, "PNG")
            return np.frombuffer(file.getvalue(), dtype=np.uint8).copy()
        self.jpeg_fallbacks += 1
        Image.fromarray(slot.np_out).save(file, "JPEG", quality=self.jpeg["quality"], subsampling={"444": 0, "420": 2}[self.jpeg["subsampling"]])
        return np.frombuffer(file.getvalue(), dtype=np.uint8).copy()

    def _allocate(self, h: int, w: int) -> None:
        self._drain()
        if self._compute is None:
            self._compute = torch.cuda.current_stream(self.device)
            self._up, self._down = torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
        else:                        # the old slots' device buffers return to the allocator: nothing may still be reading them
            for st in (self._up, self._compute, self._down):
                st.synchronize()
        s = self.model.upscale_factor
        self._plan = None
        in_shape, out_shape = self._fmt.shapes(h, w, s, self.outscale)     # an odd 4:2:0 result: ValueError before anything is allocated
        self._plan = _resize_plan(h, w, s, self.outscale, self.device)
        with torch.cuda.device(self.device):
            self._slots = [_Slot(in_shape, out_shape, self.device, self._fmt.dtype, self._fmt.out_dtype) for _ in range(self.depth)]
        self._shape, self._next = (h, w), 0

    def submit(self, frame: np.ndarray) -> None:
        if self._closed:
            raise RuntimeError("FrameStream: closed")
        size = self._fmt.size(frame)
        if len(self._pending) >= self.depth:
            raise RuntimeError(f"FrameStream: {self.depth} frames are pending already; take a result() first")
        if size != self._shape:
            self._allocate(*size)
        slot = self._slots[self._next]
        self._next = (self._next + 1) % self.depth
        np.copyto(slot.np_in, frame)                 # (the slot's previous upload finished before its result was handed back)
        with torch.cuda.stream(self._up):
            if slot.used:
                self._up.wait_event(slot.computed)   # the tail of the previous frame in this slot re-read dev_in
            slot.dev_in.copy_(slot.pin_in, non_blocking=True)
            slot.uploaded.record(self._up)
        with torch.cuda.stream(self._compute):
            self._compute.wait_event(slot.uploaded)
            slot.dev_out = self._fmt.upscale(self.model, slot.dev_in, self.outscale, self._plan)
            slot.computed.record(self._compute)
            if self.on_device is not None:
                self.on_device(slot.dev_out)
            if self.jpeg is not None or self.png is not None:
                raw = slot.dev_out[0].numel()
                if self.png is not None:
                    from .png_encode import encode_png
                    slot.jpeg_buf, slot.jpeg_len = encode_png(slot.dev_out, capacity=min(self.png_capacity or raw, raw), **self.png)
                else:
                    from .jpeg_encode import encode_jpeg
                    slot.jpeg_buf, slot.jpeg_len = encode_jpeg(slot.dev_out, capacity=min(self.jpeg_capacity or raw, raw), **self.jpeg)
                if slot.pin_len is None:
                    slot.pin_len, slot.encoded = torch.empty(1, dtype=torch.int64, pin_memory=True), torch.cuda.Event()
                slot.encoded.record(self._compute)
        with torch.cuda.stream(self._down):
            if self.jpeg is not None or self.png is not None:      # the length alone; the bytes follow when result() knows how many (_take_jpeg)
                self._down.wait_event(slot.encoded)
                slot.pin_len.copy_(slot.jpeg_len, non_blocking=True)
            else:
                self._down.wait_event(slot.computed)
                slot.pin_out.copy_(slot.dev_out, non_blocking=True)
            slot.downloaded.record(self._down)
        slot.used = True
        self._pending.append(slot)

    def result(self, copy: bool = True) -> np.ndarray:
        """The oldest result not yet taken (see the class docstring for `copy=False`)."""
        if self._ready:
            return self._ready.popleft()
        if not self._pending:
            raise RuntimeError("FrameStream: no frame is pending")
        return self._take(self._pending.popleft(), copy)

    def map(self, frames: Iterable[np.ndarray], copy: bool = True) -> Iterator[np.ndarray]:
        """Results of `frames` in input order, `depth` frames in flight."""
        for frame in frames:
            while self._ready or len(self._pending) >= self.depth:
                yield self.result(copy)
            self.submit(frame)
        while len(self):
            yield self.result(copy)

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        if self._compute is not None:
            for st in (self._up, self._compute, self._down):
                st.synchronize()
        self._pending.clear()
        self._ready.clear()
        self._slots = []

    def __enter__(self) -> "FrameStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def _check_host_frame(frame, fmt: PixelFormat) -> None:
    """ValueError unless `frame` is a host frame of this format: HxWx3 bytes ("rgb24"), else [3H/2, W] words of the format's depth."""
    rgb = fmt.layout is None
    if isinstance(frame, np.ndarray) and frame.dtype == fmt.np_dtype:
        if (frame.ndim == 3 and frame.shape[2] == 3 and min(frame.shape) >= 1) if rgb else (frame.ndim == 2 and _yuv_hw(frame.shape) is not None):
            return
    got = f"{frame.dtype} {frame.shape}" if isinstance(frame, np.ndarray) else type(frame).__name__
    want = "an HxWx3 uint8 ndarray" if rgb else (f"a [3H/2, W] {fmt.np_dtype} ndarray with H and W even "
                                                  f"(a {'10-bit ' if fmt.bits == 10 else ''}4:2:0 frame)")
    raise ValueError(f"FrameStream: expected {want}, got {got}")


class _StreamFormat:
    """What FrameStream asks of its pixel format, answered from its row of PIXEL_FORMATS: `dtype` of the slots; `size(frame)` checks
    a host frame and returns its (h, w); `shapes(h, w, s, outscale)` the slots' (in_shape, out_shape), ValueError for a result the
    format cannot hold; `upscale(model, dev_in, outscale, plan)` runs one slot on the device.  `out_name`, `out_matrix`: the
    destination, None for the source's -- then everything is as it was with one format; else `out_dtype` and the output shape are
    the destination's and a slot runs `upscale_frames`."""

    def __init__(self, name: str, matrix: str, out_name: Optional[str] = None, out_matrix: Optional[str] = None) -> None:
        self.name, self.matrix, self.fmt = name, matrix, PIXEL_FORMATS[name]
        self.dtype, self.rgb = self.fmt.torch_dtype, self.fmt.layout is None
        self.out_name = name if out_name is None else out_name
        self.out_fmt = PIXEL_FORMATS[self.out_name]
        self.out_dtype, self.out_rgb = self.out_fmt.torch_dtype, self.out_fmt.layout is None
        self.out_matrix = matrix if out_matrix is None and not self.out_rgb else out_matrix
        # one format on both sides (rgb24 has no matrix to differ in): the same-format functions, as before there was a destination
        self.mixed = self.out_name != name or (not self.rgb and self.out_matrix != matrix)

    def size(self, frame):
        _check_host_frame(frame, self.fmt)
        return frame.shape[:2] if self.rgb else _yuv_hw(frame.shape)

    def shapes(self, h, w, s, outscale):
        out_h, out_w = output_size(h, w, s, outscale) if self.out_rgb else yuv420_output_size(h, w, s, outscale, "FrameStream")
        return (h, w, 3) if self.rgb else (h * 3 // 2, w), (out_h, out_w, 3) if self.out_rgb else (out_h * 3 // 2, out_w)

    def upscale(self, model, dev_in, outscale, plan):
        if self.mixed:
            return upscale_frames(model, dev_in, (self.name, None if self.rgb else self.matrix),
                                  (self.out_name, None if self.out_rgb else self.out_matrix), outscale=outscale, plan=plan)
        if self.rgb:
            return upscale_u8(model, dev_in, outscale=outscale, plan=plan)
        fn = upscale_yuv420 if self.fmt.bits == 8 else upscale_yuv420p10
        return fn(model, dev_in, self.name, self.matrix, outscale=outscale, plan=plan)
