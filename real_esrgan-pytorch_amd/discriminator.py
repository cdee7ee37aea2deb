"""U-Net discriminator with spectral norm (reference model.py:135-203) on the gfx950 kernels.

Same constructor, forward semantics ([N,3,H,W] -> [N,1,H,W] logits, H,W divisible by 8) and state_dict
keys as the reference (`conv1.*`, `{down_block1..3,up_block1..3,conv2,conv3}.0.{weight_orig,weight_u,
weight_v}`, `conv4.*`): the parameter containers are literally `spectral_norm(nn.Conv2d(...))` objects
built in the reference's order, so the init RNG stream is identical; their Python forward is never used.

forward / backward are ONE C-ABI call each (`resr_discriminator_forward` / `_backward`, include/resr.h;
plan and launch order in csrc/disc_native.hip): spectral norm (one power iteration per training-mode
forward, u / v updated in place like torch's hook, 1/sigma folded into the packed weights on the device),
MFMA implicit-GEMM convolutions with all 64-channel output groups of a layer in one launch, the three
4x4 / stride-2 convolutions as sparse-tap 3x3 convolutions over the space-to-depth image, bilinear x2,
skip adds and LeakyReLU masks; backward mirrors it and maps the weight gradients back to `weight_orig`.
Parameters are views into one flat fp32 arena, the spectral-norm vectors into another; every call works
inside one pooled workspace (activations, this call's u / v / sigma and packed weights, scratch).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import torch
from torch import nn
from torch.nn.utils import spectral_norm

from . import _arena, _lib
from .model import _f16_backward_flag, _precision_to_dtype


class _DWorkspace(_arena.Workspace):
    """One workspace + the pack table that points into it."""

    def __init__(self, nbytes: int, device, desc) -> None:
        # the head: 1 / sigma + the gradient pre-scale slot with its sticky back-off words, zero once (include/resr.h)
        super().__init__(nbytes, device, 256)
        L = _lib.lib()
        host = _lib.fetch_pack_table(lambda out, cap: L.resr_discriminator_pack_table(C.byref(desc), _lib.ptr(self.buf), out, cap),
                                     "resr_discriminator_pack_table")
        self.table = _lib.upload_chunks(host, device)
        self.n_chunks = len(host)


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module: "Discriminator", training: bool, x: torch.Tensor, *params: torch.Tensor):
        y, desc, ws = module._run_forward(x, training)
        ctx.module, ctx.desc, ctx.ws = module, desc, ws
        ctx.x_needs_grad = x.requires_grad
        ctx.param_needs = [p.requires_grad for p in params]
        if training:     # frees the workspace when backward has run, or when the graph is dropped without one
            ctx._token = _arena.GraphToken(ws)
        return y

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        grads, gx = ctx.module._run_backward(ctx.desc, ctx.ws, gy.contiguous().float(), ctx.x_needs_grad, any(ctx.param_needs))
        ctx._token.finish()
        return (None, None, gx) + tuple(g if need else None for g, need in zip(grads, ctx.param_needs))


class Discriminator(nn.Module):
    """Reference `Discriminator()` (model.py:135-203).  Extra keyword `precision`, as for `Generator`: "fast" (f16 MFMA, fp32
    accumulate), "exact16" (split-operand f16 MFMA on hi/lo pairs: fp32-class results, the mode that meets the 1e-3 parity
    tolerance) or "strict" (f32 MFMA); anything else raises.

    `f16_backward` (exact16 only; default $RESR_X2_F16_BACKWARD = "1", read for exact16 modules only): the output-parity
    operating point, the discriminator's counterpart of the generator's x2_plan bit 8.  The forward -- logits, u / v updates --
    is exact16's, bit for bit; the backward pass is fast mode's f16 pass on the hi halves of the saved pair activations, with
    an f16 packing of the same weights and this call's sigma (`resr_discriminator_backward_f16`).  Gradients are then in fast
    mode's class.  An explicit True with "fast" or "strict" raises ValueError."""

    def __init__(self, precision: Optional[str] = None, f16_backward: Optional[bool] = None) -> None:
        super().__init__()
        self.precision = precision or os.environ.get("RESR_PRECISION", "fast")
        self._dtype = _precision_to_dtype(self.precision)          # ValueError for an unknown precision: never a silent downgrade
        self.f16_backward = _f16_backward_flag(self.precision, f16_backward, "Discriminator")
        self.conv1 = nn.Conv2d(3, 64, (3, 3), (1, 1), (1, 1))
        self.down_block1 = nn.Sequential(spectral_norm(nn.Conv2d(64, 128, (4, 4), (2, 2), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.down_block2 = nn.Sequential(spectral_norm(nn.Conv2d(128, 256, (4, 4), (2, 2), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.down_block3 = nn.Sequential(spectral_norm(nn.Conv2d(256, 512, (4, 4), (2, 2), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.up_block1 = nn.Sequential(spectral_norm(nn.Conv2d(512, 256, (3, 3), (1, 1), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.up_block2 = nn.Sequential(spectral_norm(nn.Conv2d(256, 128, (3, 3), (1, 1), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.up_block3 = nn.Sequential(spectral_norm(nn.Conv2d(128, 64, (3, 3), (1, 1), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.conv2 = nn.Sequential(spectral_norm(nn.Conv2d(64, 64, (3, 3), (1, 1), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.conv3 = nn.Sequential(spectral_norm(nn.Conv2d(64, 64, (3, 3), (1, 1), (1, 1), bias=False)), nn.LeakyReLU(0.2, True))
        self.conv4 = nn.Conv2d(64, 1, (3, 3), (1, 1), (1, 1))
        self._flat: Optional[torch.Tensor] = None       # fp32 parameter arena (named_parameters order)
        self._uv: Optional[torch.Tensor] = None         # fp32 spectral-norm arena (named_buffers order)
        self._workspaces: Dict[tuple, List[_DWorkspace]] = {}
        self.grad_hook = None   # optional callable(flat_grad) after a backward that produced weight gradients

    # ---- arenas ---------------------------------------------------------------------------------------------
    def _ordered_params(self) -> List[nn.Parameter]:
        return [p for _, p in self.named_parameters()]

    def flat_parameters(self) -> torch.Tensor:
        params = self._ordered_params()
        if not _arena.is_arena(self._flat, params):
            if sum(p.numel() for p in params) != _lib.lib().resr_discriminator_param_count():
                raise RuntimeError("Discriminator: parameter count differs from the native plan")
            self._flat = _arena.build(self.named_parameters(), lambda name, p, view: setattr(p, "data", view))
            self._workspaces.clear()
        return self._flat

    def flat_parameter(self) -> nn.Parameter:
        """One leaf Parameter aliasing the whole fp32 arena (as `Generator.flat_parameter`): `optim.Adam([d.flat_parameter()],
        fused=True)` and the GradScaler's unscale / inf check are single launches, and the autograd graph carries ONE parameter
        input instead of 19 (no per-tensor AccumulateGrad copies / adds: the two backward passes of a GAN step,
        train_realesrgan.py:503-516, meet in one `add_` over the arena).  After this call backward ACCUMULATES the gradient arena
        into this Parameter's `.grad` (autograd semantics) and hands out no per-tensor gradients; `zero_grad()` clears it; setting
        `requires_grad` on the module's parameters (the frozen discriminator of the generator step, :465-466) is mirrored onto it
        by `requires_grad_`.  `state_dict()` is unchanged."""
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

    def flat_uv(self) -> torch.Tensor:
        """The spectral-norm vectors (`weight_u`, `weight_v` of the eight normalised convs, named_buffers order) as views of
        one arena: the native forward updates them in place, a data-parallel broadcast moves them in one message."""
        named = list(self.named_buffers())
        if not _arena.is_arena(self._uv, [b for _, b in named]):
            if sum(b.numel() for _, b in named) != _lib.lib().resr_discriminator_uv_count():
                raise RuntimeError("Discriminator: spectral-norm buffer count differs from the native plan")

            def assign(name: str, b: torch.Tensor, view: torch.Tensor) -> None:
                mod, leaf = name.rsplit(".", 1)
                setattr(self.get_submodule(mod), leaf, view)
            self._uv = _arena.build(named, assign)
        return self._uv

    # ---- C-ABI plumbing ---------------------------------------------------------------------------------------
    def _workspace(self, desc, device) -> _DWorkspace:
        # the output-parity backward leaves f16 weights in a training workspace's packed region: a pool of its own
        key = (desc.n, desc.h, desc.w, desc.training, desc.dtype) + ((True,) if self.f16_backward and desc.training else ())

        def make() -> _DWorkspace:
            nbytes = _lib.lib().resr_discriminator_workspace_bytes(C.byref(desc))
            if nbytes == 0:
                raise RuntimeError("Discriminator: expected [N,3,H,W] with H, W divisible by 8")
            return _DWorkspace(nbytes, device, desc)
        return _arena.take(self._workspaces, key, device, make)

    def _run_forward(self, x: torch.Tensor, training: bool):
        L = _lib.lib()
        _lib.require_cuda(x, "Discriminator.forward")
        flat, uv = self.flat_parameters(), self.flat_uv()
        _lib.require_cuda(flat, "Discriminator parameters")
        n, c, h, w = x.shape
        if c != 3 or (h % 8) or (w % 8):
            raise RuntimeError("Discriminator: expected [N,3,H,W] with H, W divisible by 8")
        xc = x.detach().float().contiguous()
        desc = _lib.DiscriminatorDesc(n, h, w, self._dtype, 1 if training else 0, 1 if self.training else 0)
        ws = self._workspace(desc, xc.device)
        y = torch.empty((n, 1, h, w), dtype=torch.float32, device=xc.device)
        _lib.check(L.resr_discriminator_forward(C.byref(desc), _lib.ptr(xc), _lib.ptr(flat), _lib.ptr(uv), _lib.ptr(ws.table), ws.n_chunks,
                                                _lib.ptr(ws.buf), ws.buf.numel(), _lib.ptr(y), _lib.stream_ptr(xc)),
                   "resr_discriminator_forward")
        return y, desc, ws

    def _run_backward(self, desc, ws: _DWorkspace, gy: torch.Tensor, need_gx: bool, need_w: bool):
        L = _lib.lib()
        flat = self.flat_parameters()
        # a fresh arena per backward: autograd adds the two backward passes of a GAN step (train_realesrgan.py:503-516) itself,
        # and the per-parameter views it is handed stay consecutive in memory (one all-reduce for the data-parallel exchange)
        gflat = torch.zeros_like(flat) if need_w else None
        gx = torch.empty((desc.n, 3, desc.h, desc.w), dtype=torch.float32, device=gy.device) if need_gx else None
        if self.f16_backward:
            _lib.check(L.resr_discriminator_backward_f16(C.byref(desc), _lib.ptr(gy), _lib.ptr(flat), _lib.ptr(ws.table), ws.n_chunks,
                                                         _lib.ptr(ws.buf), ws.buf.numel(), _lib.ptr(gflat), _lib.ptr(gx),
                                                         _lib.stream_ptr(gy)), "resr_discriminator_backward_f16")
        else:
            _lib.check(L.resr_discriminator_backward(C.byref(desc), _lib.ptr(gy), _lib.ptr(flat), _lib.ptr(ws.buf), ws.buf.numel(),
                                                     _lib.ptr(gflat), _lib.ptr(gx), _lib.stream_ptr(gy)), "resr_discriminator_backward")
        if not need_w:
            return [None] * len(self._ordered_params()), gx
        if self.grad_hook is not None:
            self.grad_hook(gflat)
        fp = _arena.flat_alias(self, flat)
        if fp is not None:                        # flat_parameter() mode: accumulate into the alias, no per-tensor gradients
            if fp.grad is None:
                fp.grad = gflat
            else:
                fp.grad.add_(gflat)
            return [None], gx
        return list(_arena.views(gflat, self.named_parameters()).values()), gx

    # ---- module surface -----------------------------------------------------------------------------------------
    def _forward_impl(self, x: torch.Tensor) -> torch.Tensor:
        fp = _arena.flat_alias(self, self.flat_parameters())           # the arena may have been rebuilt: the alias follows it
        params = [fp] if fp is not None else self._ordered_params()     # flat_parameter() mode: one graph input for all 19 tensors
        training = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _DiscFn.apply(self, training, x, *params)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._forward_impl(x)
