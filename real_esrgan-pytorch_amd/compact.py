"""The compact generator of upstream Real-ESRGAN (`SRVGGNetCompact`: the realesr-animevideov3 and realesr-general-x4v3
models) on the MI355X conv kernels: inference by default, trainable on request.

Same constructor, module tree and state_dict keys as upstream (`body` = ModuleList of conv / activation, `upsampler` =
PixelShuffle), so an official `.pth` loads with a plain `load_state_dict` (or `model.load_official_state_dict`).  `forward` is
one C-ABI call, `resr_compact_forward` (include/resr.h, csrc/compact.hip): conv 3->64 + act, num_conv x (conv 64->64 + act),
conv 64->3*s*s, pixel-shuffle, + the nearest-upsampled input.  There is no PyTorch / CPU fallback.

`SRVGGNetCompact(..., trainable=True)` ("fast" or "strict") adds the native backward pass: a forward with grad enabled and an
input or parameter that requires grad runs `resr_compact_forward_train` -- the same convolutions on a plain epilogue, every
pre-activation and activation kept in a workspace the graph owns -- and its backward `resr_compact_backward` (csrc/compact.hip,
compact_train.hip; DESIGN, "Compact generator: training").  Every other call, and every call of a model built without the flag,
takes the inference path below unchanged; without the flag a forward that would need a graph raises.  The training surface is
`Generator`'s: `grad_hook` (the data-parallel exchange, `train.DataParallel.attach`), `flat_parameter()` / `flat_grad()` (one
optimiser tensor, one graph input), and the train scripts reach the model through `config.build_generator` ($RESR_G_ARCH=compact).

Every forward checks its own input, allocates its own result and goes through one call path (`_call`).

`forward_u8` is the same launch sequence for uint8 HWC frames (`resr_compact_forward_u8`, csrc/frames.hip): the `/ 255` of the
way in is fused into the first kernel and the `* 255`, clamp and truncation of `imgproc.tensor_to_image` into the last, so its
result equals `tensor_to_image(forward(float frame))` bit for bit and a quarter of the output bytes leave the device.  It is
forward only as well (frames.py builds the pipelined host-to-host stream on it).

`forward_yuv420` is that sequence for YUV 4:2:0 frames (I420 / NV12, `resr_compact_forward_yuv420`): the integer colour conversions
of frames.py fused into the same two kernels, so its result equals `rgb_to_yuv420_np(forward_u8(yuv420_to_rgb_np(f)))` bit for bit.
`forward_yuv420p10` is the same for 10-bit frames.  Both take `outscale` as `forward_u8` does (`resr_compact_forward_yuv420_scaled` /
`_yuv420p10_scaled`, csrc/image_resize.hip): the resized tail with a YUV 4:2:0 output stage, still one launch sequence.
`forward_yuv420_mixed` is the sequence with a source and a destination format of their own (`resr_compact_forward_yuv420_mixed`, `_scaled`):
8 bits in and 10 out, NV12 / P010 in and planar out, BT.601 in and BT.709 out -- the head reads the source, the tail writes the destination.

`forward_image` is the sequence for grey, RGB and RGBA images of 8 or 16 bits (`resr_compact_forward_image`): the network runs on the
colour (or replicated grey) images and, for RGBA, on the alpha planes as grey images behind them; the head reads the image's own
words and the tail writes them, grey and alpha through the fixed-point grey of their three levels (frames.py, IMAGE MODES).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import torch
from torch import nn

from . import _arena, _lib
from .model import _precision_to_dtype

__all__ = ["SRVGGNetCompact"]

_ACTS = {"prelu": _lib.COMPACT_PRELU, "leakyrelu": _lib.COMPACT_LRELU, "relu": _lib.COMPACT_RELU}


class _CompactFn(torch.autograd.Function):
    """One training graph of a trainable SRVGGNetCompact: forward saves into a workspace of its own, backward reads it."""

    @staticmethod
    def forward(ctx, module: "SRVGGNetCompact", x: torch.Tensor, *params: torch.Tensor):
        y, desc, ws, packed = module._run_forward_train(x)
        ctx.module, ctx.desc, ctx.ws, ctx.packed = module, desc, ws, packed
        ctx.x_dtype = x.dtype
        ctx.one_tensor = len(params) == 1 and params[0] is _arena.flat_alias(module)   # flat_parameter() mode: the alias stands for all
        ctx._token = _arena.GraphToken(ws)   # the workspace is this graph's until its backward has run or the graph is dropped
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        if not ctx._token.open:
            raise RuntimeError("SRVGGNetCompact: this graph's backward has run already and its workspace was given back "
                               "(run the forward again; retain_graph is not supported on the native pass)")
        grads, gx = ctx.module._run_backward(ctx.desc, ctx.ws, ctx.packed, gy.contiguous().float(), ctx.needs_input_grad[1],
                                             ctx.needs_input_grad[2:], ctx.one_tensor)
        ctx._token.finish()
        return (None, gx if gx is None else gx.to(ctx.x_dtype)) + tuple(grads)


class SRVGGNetCompact(nn.Module):
    """SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu") as upstream.

    Keyword `precision`: "fast" (f16 MFMA), "exact16" (split-operand f16 pairs, three stages per chunk, fp32-class results) or
    "strict" (f32 MFMA); default $RESR_PRECISION, else "fast" -- the rule of `Generator`.
    forward(x [N,3,H,W] float, NCHW or channels_last, any H, W >= 1) -> [N,3,sH,sW] fp32 NCHW, not clamped.
    Keyword `trainable` (default False): False = forward only -- a call with grad enabled and an input or parameter that requires
    grad raises (wrap inference in torch.no_grad()).  True ("fast" or "strict"; "exact16" is a ValueError): such a call of `forward`
    is differentiable -- gradients of every parameter that requires grad and of x, each backward handing autograd views of a fresh
    flat fp32 tensor (plain accumulation into `.grad`); fast mode's gradients do not depend on the caller's loss scale (the lift of
    `Generator`).  Calls that need no graph, and the frame entries (which keep raising under grad mode), are the inference path.
    """

    def __init__(self, num_in_ch: int = 3, num_out_ch: int = 3, num_feat: int = 64, num_conv: int = 16, upscale: int = 4,
                 act_type: str = "prelu", precision: Optional[str] = None, trainable: bool = False) -> None:
        super().__init__()
        if num_in_ch != 3 or num_out_ch != 3:
            raise ValueError(f"SRVGGNetCompact: num_in_ch = num_out_ch = 3 on this path, got {num_in_ch}, {num_out_ch}")
        if num_feat != 64:
            raise ValueError(f"SRVGGNetCompact: num_feat must be 64 (the conv kernels' channel tiles), got {num_feat}")
        if isinstance(num_conv, bool) or not isinstance(num_conv, int) or not 0 <= num_conv <= 4096:
            raise ValueError(f"SRVGGNetCompact: num_conv must be an int in [0, 4096], got {num_conv!r}")
        if isinstance(upscale, bool) or upscale not in (1, 2, 3, 4):
            raise ValueError(f"SRVGGNetCompact: upscale must be 1, 2, 3 or 4, got {upscale!r}")
        if act_type not in _ACTS:
            raise ValueError(f"SRVGGNetCompact: act_type must be 'prelu', 'leakyrelu' or 'relu', got {act_type!r}")
        self.num_in_ch, self.num_out_ch, self.num_feat = num_in_ch, num_out_ch, num_feat
        self.num_conv, self.upscale, self.act_type = num_conv, upscale, act_type
        self.precision = precision or os.environ.get("RESR_PRECISION", "fast")
        self._dtype = _precision_to_dtype(self.precision)
        self.trainable = bool(trainable)
        if self.trainable and self._dtype == _lib.RESR_F16X2:
            raise ValueError("SRVGGNetCompact: trainable=True takes precision 'fast' or 'strict' (exact16 training is not built)")

        # upstream's module tree (same construction order, hence the same init under the same seed)
        self.body = nn.ModuleList()
        self.body.append(nn.Conv2d(num_in_ch, num_feat, 3, 1, 1))
        self.body.append(self._activation(num_feat))
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(num_feat, num_feat, 3, 1, 1))
            self.body.append(self._activation(num_feat))
        self.body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(upscale)

        self._flat: Optional[torch.Tensor] = None
        self._packed: Optional[torch.Tensor] = None
        self._table_dev: Optional[tuple] = None
        self._workspaces: Dict[tuple, torch.Tensor] = {}
        # training graphs (trainable=True): the packing with the transposed chunks, and pooled workspaces a live graph owns
        self._packed_train: Optional[torch.Tensor] = None
        self._table_train: Optional[tuple] = None
        self._train_workspaces: Dict[tuple, List[_arena.Workspace]] = {}
        self.grad_hook = None   # optional callable(flat_grad) after a backward that produced weight gradients (data-parallel all-reduce)

    def _activation(self, num_feat: int) -> nn.Module:
        if self.act_type == "prelu":
            return nn.PReLU(num_parameters=num_feat)
        if self.act_type == "leakyrelu":
            return nn.LeakyReLU(negative_slope=0.1, inplace=True)
        return nn.ReLU(inplace=True)

    # ---- what the tiler needs (tiling.py; Generator defines the same) ----------------------------------------------------
    @property
    def upscale_factor(self) -> int:
        return self.upscale

    @property
    def out_channels(self) -> int:
        return self.num_out_ch

    pixel_unshuffle_factor = 1   # every conv runs at the input's resolution
    conv_scale = 1               # ... so the largest conv tensor is LR-sized (the tail's shuffle + residual is 64-bit indexed)

    @property
    def receptive_radius(self) -> int:
        """LR pixels a window needs around a tile for the tiled output to equal whole-frame output: one per conv."""
        return self.num_conv + 2

    # ---- flat arena (as Generator: parameters are views of one fp32 buffer in named_parameters order) -------------------
    def _ordered_params(self) -> List[nn.Parameter]:
        return [p for _, p in self.named_parameters()]

    def flat_parameters(self) -> torch.Tensor:
        """The fp32 arena all parameters are views of (named_parameters order = resr_compact_forward's layout)."""
        if not _arena.is_arena(self._flat, self._ordered_params()):
            self._flat = _arena.build(self.named_parameters(), lambda name, p, view: setattr(p, "data", view))
            self._packed = None
            self._table_dev = None
            self._workspaces.clear()
            self._packed_train = None
            self._table_train = None
            self._train_workspaces.clear()
            _arena.flat_alias(self, self._flat)   # the arena was rebuilt (`.to()`, EMA.apply_shadow / restore): the alias follows it
        return self._flat

    def flat_parameter(self) -> nn.Parameter:
        """One leaf Parameter aliasing the whole fp32 arena (as `Generator.flat_parameter`, `Discriminator.flat_parameter`):
        `optim.Adam([g.flat_parameter()], fused=True)` and the GradScaler's unscale / inf check are single launches, and a training
        graph carries ONE parameter input instead of 3 * num_conv + 5 (PReLU).  Once it exists (and requires grad) a training
        `forward` hands autograd this tensor alone and backward returns the fresh flat gradient tensor for it: `.grad` of the alias
        accumulates by autograd's own add, the per-tensor Parameters receive no gradients; `zero_grad()` clears it and
        `requires_grad_` is mirrored onto it.  `parameters()`, `state_dict()` and their key order are unchanged; on a model built
        without `trainable` it may be held by an optimiser and changes nothing about the guard."""
        return _arena.flat_alias(self, self.flat_parameters(), create=True)

    def flat_grad(self) -> Optional[torch.Tensor]:
        fp = _arena.flat_alias(self)
        return None if fp is None else fp.grad

    def zero_grad(self, set_to_none: bool = True) -> None:
        super().zero_grad(set_to_none=set_to_none)
        fp = _arena.flat_alias(self)
        if fp is not None and fp.grad is not None:
            if set_to_none:
                fp.grad = None
            else:
                fp.grad.zero_()

    def requires_grad_(self, requires_grad: bool = True):
        fp = _arena.flat_alias(self)
        if fp is not None:
            fp.requires_grad_(requires_grad)
        return super().requires_grad_(requires_grad)

    # ---- C-ABI plumbing ---------------------------------------------------------------------------------------------------
    def _desc(self, n: int, h: int, w: int) -> _lib.CompactDesc:
        return _lib.CompactDesc(n, h, w, self.num_conv, self.upscale, _ACTS[self.act_type], self._dtype, 0)

    def _pack(self, desc: _lib.CompactDesc, flat: torch.Tensor) -> None:
        """One resr_pack_weights launch per forward: a load_state_dict or an in-place edit is always seen (graph replays too)."""
        L = _lib.lib()
        if self._table_dev is None or self._table_dev[0].device != flat.device:
            host = _lib.fetch_pack_table(lambda out, cap: L.resr_compact_pack_table(C.byref(desc), out, cap), "resr_compact_pack_table")
            self._table_dev = (_lib.upload_chunks(host, flat.device), len(host))
        nbytes = L.resr_compact_packed_bytes(C.byref(desc))
        if self._packed is None or self._packed.numel() < nbytes or self._packed.device != flat.device:
            self._packed = torch.zeros(nbytes, dtype=torch.uint8, device=flat.device)
        raw, n = self._table_dev
        _lib.check(L.resr_pack_weights(_lib.ptr(raw), n, _lib.ptr(flat), _lib.ptr(self._packed), self._dtype,
                                       _lib.stream_ptr(flat)), "resr_pack_weights")

    def _workspace(self, desc: _lib.CompactDesc, device) -> torch.Tensor:
        key = (desc.n, desc.h, desc.w, desc.dtype, str(device))
        ws = self._workspaces.get(key)
        if ws is None:
            nbytes = _lib.lib().resr_compact_workspace_bytes(C.byref(desc))
            if nbytes == 0:
                raise RuntimeError(f"resr_compact_workspace_bytes: unsupported shape {desc.n}x{desc.h}x{desc.w} for precision "
                                   f"{self.precision!r} (exact16 takes at most 2^24 pixels per call: use tiling.TiledGenerator)")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._workspaces[key] = ws
        return ws

    def _guard(self, x: Optional[torch.Tensor] = None) -> None:
        if torch.is_grad_enabled() and ((x is not None and x.requires_grad) or any(p.requires_grad for p in self._ordered_params())):
            raise RuntimeError("SRVGGNetCompact: the compact generator's backward pass is not implemented on the MI355X path; "
                               "run inference under torch.no_grad() (or with requires_grad_(False) parameters)")

    def _call(self, entry: str, src: torch.Tensor, n: int, h: int, w: int, y: torch.Tensor, *extra, after_src=()) -> torch.Tensor:
        """What every forward shares once its own input is checked: the arena, the descriptor of n LR frames h x w, packing, the
        workspace, then `entry` (its ends `src` and `y`; `extra`: the arguments between y and the stream; `after_src`: those between
        src and the parameters, the mixed entries' source descriptor)."""
        flat = self.flat_parameters()
        _lib.require_cuda(flat, "SRVGGNetCompact parameters")
        desc = self._desc(n, h, w)
        self._pack(desc, flat)
        ws = self._workspace(desc, src.device)
        _lib.check(getattr(_lib.lib(), entry)(C.byref(desc), _lib.ptr(src), *after_src, _lib.ptr(flat), _lib.ptr(self._packed), _lib.ptr(ws),
                                              ws.numel(), _lib.ptr(y), *extra, _lib.stream_ptr(src)), entry)
        return y

    # ---- training graphs (trainable=True) ---------------------------------------------------------------------------------
    def _run_forward_train(self, x: torch.Tensor):
        """resr_compact_forward_train on a workspace no live graph holds: (y, descriptor, workspace, packed buffer).  The packed
        buffer is the module's, as `Generator`'s: graphs that are live together share it, so their backward passes read the weights
        of the latest forward (the same ones, unless an optimizer stepped between a forward and its backward)."""
        L = _lib.lib()
        flat = self.flat_parameters()
        _lib.require_cuda(flat, "SRVGGNetCompact parameters")
        xc = x.detach().float().contiguous()
        n, _, h, w = xc.shape
        desc = self._desc(n, h, w)
        if self._table_train is None or self._table_train[0].device != flat.device:
            host = _lib.fetch_pack_table(lambda out, cap: L.resr_compact_train_pack_table(C.byref(desc), out, cap), "resr_compact_train_pack_table")
            self._table_train = (_lib.upload_chunks(host, flat.device), len(host))
        nbytes = L.resr_compact_train_packed_bytes(C.byref(desc))
        if self._packed_train is None or self._packed_train.numel() < nbytes or self._packed_train.device != flat.device:
            self._packed_train = torch.zeros(nbytes, dtype=torch.uint8, device=flat.device)
        raw, nchunks = self._table_train     # one pack launch per forward; the backward reads the same buffer
        _lib.check(L.resr_pack_weights(_lib.ptr(raw), nchunks, _lib.ptr(flat), _lib.ptr(self._packed_train), self._dtype,
                                       _lib.stream_ptr(flat)), "resr_pack_weights")

        def make() -> _arena.Workspace:
            nb = L.resr_compact_train_workspace_bytes(C.byref(desc))
            if nb == 0:
                raise RuntimeError(f"resr_compact_train_workspace_bytes: unsupported shape {n}x{h}x{w} ({(L.resr_last_error() or b'').decode()})")
            return _arena.Workspace(nb, xc.device, int(L.resr_compact_train_state_bytes(C.byref(desc))))   # the pre-scale slot: zero once
        ws = _arena.take(self._train_workspaces, (n, h, w, desc.dtype), xc.device, make)
        s = self.upscale
        y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=xc.device)
        _lib.check(L.resr_compact_forward_train(C.byref(desc), _lib.ptr(xc), _lib.ptr(flat), _lib.ptr(self._packed_train), _lib.ptr(ws.buf),
                                                ws.buf.numel(), _lib.ptr(y), _lib.stream_ptr(xc)), "resr_compact_forward_train")
        return y, desc, ws, self._packed_train

    def _run_backward(self, desc, ws: _arena.Workspace, packed: torch.Tensor, gy: torch.Tensor, need_gx: bool, need_params,
                      one_tensor: bool = False):
        """resr_compact_backward into a fresh flat gradient tensor: per-parameter views of it (None where not needed), gx or None.
        `grad_hook` sees the flat tensor first, once, when any parameter gradient is wanted.  `one_tensor` (the graph's parameter
        input is the `flat_parameter()` alias): the flat tensor itself is the one gradient handed back."""
        flat = self.flat_parameters()
        grad = torch.empty_like(flat)
        gx = torch.empty((desc.n, self.num_in_ch, desc.h, desc.w), dtype=torch.float32, device=gy.device) if need_gx else None
        _lib.check(_lib.lib().resr_compact_backward(C.byref(desc), _lib.ptr(gy), _lib.ptr(flat), _lib.ptr(packed), _lib.ptr(ws.buf),
                                                    ws.buf.numel(), _lib.ptr(grad), _lib.ptr(gx), _lib.stream_ptr(gy)), "resr_compact_backward")
        if self.grad_hook is not None and any(need_params):
            self.grad_hook(grad)
        if one_tensor:
            return [grad if need_params[0] else None], gx
        views = _arena.views(grad, self.named_parameters()).values()
        return [g if need else None for g, need in zip(views, need_params)], gx

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # grad mode is off inside autograd.Function.forward: whether this call builds a graph is decided here
        params = self._ordered_params()
        if self.trainable:
            fp = _arena.flat_alias(self, self.flat_parameters())
            if fp is not None and fp.requires_grad:   # flat_parameter() mode: one graph input for all tensors (a frozen alias: the per-tensor flags decide)
                params = [fp]
        training = self.trainable and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        if not training:
            self._guard(x)
        _lib.require_cuda(x, "SRVGGNetCompact.forward")
        if x.dim() != 4 or x.shape[1] != self.num_in_ch:
            raise RuntimeError(f"SRVGGNetCompact: expected an [N,{self.num_in_ch},H,W] input, got {tuple(x.shape)}")
        if training:
            self.flat_parameters()   # (the parameters handed to the graph are the arena's views)
            return _CompactFn.apply(self, x, *params)
        xc = x.detach().float().contiguous()   # also normalises channels_last strides
        n, _, h, w = xc.shape
        s = self.upscale
        y = torch.empty((n, self.num_out_ch, h * s, w * s), dtype=torch.float32, device=xc.device)
        return self._call("resr_compact_forward", xc, n, h, w, y)

    def forward_u8(self, frames: torch.Tensor, outscale: Optional[float] = None, plan=None) -> torch.Tensor:
        """frames uint8 [N,H,W,3] on the model's device, contiguous -> uint8 [N,H*s,W*s,3]: bit for bit
        `imgproc.tensor_to_image(self(frames / 255 as NCHW fp32))` per image (a NaN inside the net is outside that contract).
        Same guard (a call with grad enabled and parameters that require grad raises), packing and workspace caches as `forward`.

        `outscale` (a finite positive number other than the model's factor): the final size is `frames.output_size(H, W, s,
        outscale)` instead -- `resr_compact_forward_u8_scaled`: the last kernel resizes the frame it would have stored by
        r = outscale / s (the reference's `image_resize`: antialiased bicubic, csrc/image_resize.hip) tile by tile in LDS and writes
        only the resized uint8 frame; bit for bit `imgproc.image_resize_native(self(float frames), r, u8=True)`.  `plan`: a cached
        `imgproc.ResizePlan` for this frame size and r (FrameStream keeps one).  None or the model's factor: the path above."""
        from . import frames as _frames
        o = _frames.check_outscale(outscale, self.upscale, "SRVGGNetCompact.forward_u8")
        self._guard()
        _lib.require_cuda(frames, "SRVGGNetCompact.forward_u8")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != self.num_in_ch:
            raise RuntimeError(f"SRVGGNetCompact.forward_u8: expected a uint8 [N,H,W,{self.num_in_ch}] tensor, got "
                               f"{frames.dtype} {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise RuntimeError("SRVGGNetCompact.forward_u8: frames must be contiguous (HWC bytes, as an image decoder leaves them)")
        n, h, w, _ = frames.shape
        return self._frame_tail("resr_compact_forward_u8", frames, n, h, w, lambda oh, ow: (n, oh, ow, self.num_out_ch), torch.uint8, o, plan,
                                "SRVGGNetCompact.forward_u8")

    def _frame_tail(self, entry: str, src: torch.Tensor, n: int, h: int, w: int, shape, dtype, o, plan, what: str, *desc, after_src=()) -> torch.Tensor:
        """What the frame entries share once their own input is checked (n: the network's batch; `shape(out_h, out_w)`: the
        result's; `desc`, `after_src`: the entry's descriptors, as `_call` places them).  o None: `entry` at the model's factor.
        Else `entry`_scaled with the checked plan of `_scaled_plan`, the result of the plan's size."""
        s = self.upscale
        if o is None:
            return self._call(entry, src, n, h, w, torch.empty(shape(h * s, w * s), dtype=dtype, device=src.device), *desc, after_src=after_src)
        _lib.require_cuda(self.flat_parameters(), "SRVGGNetCompact parameters")    # refused before a plan is looked at
        plan = self._scaled_plan(src, h, w, o, plan, what)
        y = torch.empty(shape(plan.out_h, plan.out_w), dtype=dtype, device=src.device)
        return self._call(entry + "_scaled", src, n, h, w, y, *plan.args(), *desc, after_src=after_src)

    def _scaled_plan(self, frames: torch.Tensor, h: int, w: int, o: float, plan, what: str):
        """The checked `imgproc.ResizePlan` of an outscale call on h x w frames: the caller's `plan` when it is one for this call,
        else a new one.  Raises before any launch (a plan for another size, a frame the reference's rule refuses)."""
        from . import frames as _frames
        s = self.upscale
        if plan is not None and ((plan.in_h, plan.in_w, plan.scale_factor) != (h * s, w * s, o / s) or plan.idx_y.device != frames.device):
            raise ValueError(f"{what}: a plan for {plan.in_h}x{plan.in_w} x {plan.scale_factor}, the call is {h * s}x{w * s} x {o / s}")
        plan = _frames._resize_plan(h, w, s, o, frames.device, plan)
        plan.check(what)
        return plan

    def _forward_yuv(self, frames: torch.Tensor, layout: str, matrix: str, outscale, plan, bits: int) -> torch.Tensor:
        """`forward_yuv420` (bits = 8) / `forward_yuv420p10` (10).  `outscale` is checked as `forward_u8` checks it, with the 4:2:0
        rule of its result -- an odd height or width is a ValueError -- before the device is looked at."""
        from . import frames as _frames
        name = _frames._yuv_name(bits)
        what, entry = "SRVGGNetCompact.forward_" + name, "resr_compact_forward_" + name
        o = _frames.check_outscale(outscale, self.upscale, what)
        hw = _frames._yuv_hw(frames.shape) if o is not None and isinstance(frames, torch.Tensor) else None
        if hw is not None:
            _frames.yuv420_output_size(hw[0], hw[1], self.upscale, o, what)
        ydesc = _frames._desc(bits, layout, matrix)
        self._guard()
        n, h, w = _frames._check_yuv(frames, what, bits)
        return self._frame_tail(entry, frames, n, h, w, lambda oh, ow: (n, oh * 3 // 2, ow), frames.dtype, o, plan, what, C.byref(ydesc))

    def forward_yuv420(self, frames: torch.Tensor, layout: str = "i420", matrix: str = "bt601", outscale: Optional[float] = None,
                       plan=None) -> torch.Tensor:
        """frames uint8 [N,3H/2,W] (YUV 4:2:0, H and W even; `layout` "i420" or "nv12", `matrix` "bt601" or "bt709": frames.py) on
        the model's device, contiguous -> uint8 [N,3sH/2,sW] in the same layout: bit for bit
        `frames.rgb_to_yuv420_np(self.forward_u8(frames.yuv420_to_rgb_np(f)))`.  `resr_compact_forward_yuv420`: the launch sequence
        of `forward_u8` with the two integer colour conversions inside its first and last kernel -- no RGB frame exists on the
        device, and half the bytes enter and leave.  Same guard, packing and workspace caches as `forward`.

        `outscale`, `plan`: as `forward_u8`'s -> uint8 [N, 3 out_h / 2, out_w] for `frames.output_size(H, W, s, outscale)`, which
        must be even both ways (ValueError) -- `resr_compact_forward_yuv420_scaled`: bit for bit
        `rgb_to_yuv420_np(self.forward_u8(yuv420_to_rgb_np(f), outscale=outscale))`, still with no RGB frame on the device.  A scale
        so small that no even tile fits the kernel's LDS is an error here; `frames.upscale_yuv420` asks first and composes."""
        return self._forward_yuv(frames, layout, matrix, outscale, plan, 8)

    def forward_yuv420p10(self, frames: torch.Tensor, layout: str = "i420p10", matrix: str = "bt601", outscale: Optional[float] = None,
                          plan=None) -> torch.Tensor:
        """frames uint16 [N,3H/2,W] (10-bit YUV 4:2:0, H and W even; `layout` "i420p10" or "p010", `matrix` "bt601" or "bt709":
        frames.py) on the model's device, contiguous -> uint16 [N,3sH/2,sW] in the same layout: bit for bit
        `frames.rgb_to_yuv420p10_np(q10(self(frames.yuv420p10_to_rgb_np(f) / 1023)))`.  `resr_compact_forward_yuv420p10`: the launch
        sequence of `forward_yuv420` with 1023 levels at both ends -- neither an RGB frame nor an fp32 copy of the input exists on
        the device.  Same guard, packing and workspace caches as `forward`.

        `outscale`, `plan`: as `forward_yuv420`'s -> uint16 [N, 3 out_h / 2, out_w] -- `resr_compact_forward_yuv420p10_scaled`: bit for
        bit `rgb_to_yuv420p10_np(q10(resize_with_plan(self(yuv420p10_to_rgb_np(f) / 1023), plan)))`; the fp32 frames of that
        composition exist as LDS tiles only."""
        return self._forward_yuv(frames, layout, matrix, outscale, plan, 10)

    def forward_yuv420_mixed(self, frames: torch.Tensor, src, dst, outscale: Optional[float] = None, plan=None) -> torch.Tensor:
        """frames [N,3H/2,W] in the YUV 4:2:0 format `src` (a `frames.FrameFormat` or a `(pix_fmt, matrix)` pair: "i420" / "nv12" uint8,
        "i420p10" / "p010" uint16; H and W even) on the model's device, contiguous -> [N,3sH/2,sW] in the format `dst`, whose depth,
        layout and matrix need not be the source's.  Bit for bit, with top = 255 or 1023 of a side,

            rgb_to_yuv_np_dst(q_dst(self(yuv_to_rgb_np_src(f) / top_src)))          q(v) = trunc(clamp(v * top, 0, top)) in fp32

        (frames.py, MIXED FRAME FORMATS).  `resr_compact_forward_yuv420_mixed`: the head of the source's depth, the convs, one tail that
        recomputes the residual from `frames` in the source's format and quantises, converts and stores in the destination's.  With
        `src == dst` this is `forward_yuv420` / `forward_yuv420p10`: the same kernels run.  "rgb24" on a side is a ValueError here --
        that end is not fused; `frames.upscale_frames` composes it.  `outscale`, `plan`: as `forward_yuv420`'s
        (`resr_compact_forward_yuv420_mixed_scaled`): the result is [N, 3 out_h / 2, out_w], resized in fp32 before `q_dst`.  Every
        ValueError (a format, a matrix, an odd frame, an odd result) comes before the device is looked at; same guard, packing and
        workspace caches as `forward`."""
        from . import frames as _frames
        what = "SRVGGNetCompact.forward_yuv420_mixed"
        a, b = _frames.frame_format(src, what), _frames.frame_format(dst, what)
        for f in (a, b):
            if f.pix_fmt == "rgb24":
                raise ValueError(f"{what}: rgb24 is not fused to a YUV format; frames.upscale_frames composes it")
        o = _frames.check_outscale(outscale, self.upscale, what)
        _frames.mixed_geometry(frames, a, b, self.upscale, o, what)
        qa, qb = _frames.format_desc(a), _frames.format_desc(b)
        self._guard()
        n, h, w = _frames._check_yuv(frames, what, a.fmt.bits)
        return self._frame_tail("resr_compact_forward_yuv420_mixed", frames, n, h, w, lambda oh, ow: (n, oh * 3 // 2, ow), b.fmt.torch_dtype, o, plan,
                                what, C.byref(qb), after_src=(C.byref(qa),))

    def forward_image(self, images: torch.Tensor, outscale: Optional[float] = None, plan=None) -> torch.Tensor:
        """images: a grey, RGB or RGBA batch -- uint8 or uint16, [N,H,W] or [N,H,W,1], [N,H,W,3], [N,H,W,4] -- on the model's device,
        contiguous -> the same dtype and trailing shape, [N,sH,sW(,C)].  Bit for bit
        `frames.rgb_to_image_np(q(self(frames.image_to_rgb_np(images) / top)), channels)` with top = 255 or 65535 and
        q(v) = trunc(clamp(v * top, 0, top)) in fp32 (frames.py, IMAGE MODES).  `resr_compact_forward_image`: the launch sequence of
        `forward_u8` on a network batch of planes * N images (RGBA: the N colour images, then the N alpha planes as grey images, as
        upstream's `alpha_upsampler="realesrgan"`) -- the head reads the image's own words, the tail writes them; no fp32 or RGB
        copy of either exists on the device.  uint8 RGB runs the kernels of `forward_u8`.  Same guard, packing and workspace caches
        as `forward`.

        `outscale`, `plan`: as `forward_u8`'s -> [N, *frames.output_size(H, W, s, outscale)(, C)] -- `resr_compact_forward_image_scaled`:
        the last kernel resizes the float frames it would have quantised by r = outscale / s, tile by tile in LDS, and quantises the
        resized sums; bit for bit `frames.to_image(imgproc.resize_with_plan(self(frames.from_image(images)), plan), C, dtype)`, whose
        fp32 frames exist as LDS tiles only (frames.py, IMAGE MODES).  A scale so small that no tile fits the kernel's LDS is an error
        here; `frames.upscale_image` asks first and composes.  None or the model's factor: the path above."""
        from . import frames as _frames
        what = "SRVGGNetCompact.forward_image"
        o = _frames.check_outscale(outscale, self.upscale, what)
        self._guard()
        n, h, w, c = _frames.check_images(images, what)
        idesc = _frames.image_desc(c, images.dtype)
        planes = 2 if c == 4 else 1
        return self._frame_tail("resr_compact_forward_image", images, planes * n, h, w, lambda oh, ow: (n, oh, ow) + tuple(images.shape[3:]),
                                images.dtype, o, plan, what, C.byref(idesc))

    def load_official_state_dict(self, checkpoint) -> None:
        """Upstream's `{"params_ema": sd}` / `{"params": sd}` (params_ema preferred) or a bare state dict (model.load_official_state_dict)."""
        from .model import load_official_state_dict
        load_official_state_dict(self, checkpoint)
