"""What `Generator`, `Discriminator` and `SRVGGNetCompact` share on the host side: the flat fp32 arena their tensors are views
of, the one-tensor alias of that arena, and the lifetime of a pooled training workspace.  Depends on nothing but torch.

What a module drops when its arena was rebuilt (packed weights, tables, pools, the gradient arena) and how it hands out
gradients is the module's own knowledge and stays next to its calls; nothing here knows who calls it.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn

Named = Iterable[Tuple[str, torch.Tensor]]


# ---- flat arena ----------------------------------------------------------------------------------------------------------
def is_arena(flat: Optional[torch.Tensor], tensors: Iterable[torch.Tensor]) -> bool:
    """True when every tensor is an fp32 view of `flat`, back to back in this order, and together they are all of it.  False
    after anything that gave a tensor new memory: `.to()`, `.double()`, a `p.data` replaced from outside (EMA.apply_shadow)."""
    if flat is None:
        return False
    base, off = flat.data_ptr(), 0
    for t in tensors:
        if t.dtype != torch.float32 or t.data_ptr() != base + 4 * off:
            return False
        off += t.numel()
    return off == flat.numel()


def build(named: Named, assign: Callable[[str, torch.Tensor, torch.Tensor], None]) -> torch.Tensor:
    """A new arena on the first tensor's device holding every tensor's values as float32, in the order given.  Each tensor is
    re-pointed through `assign(name, tensor, view)`: `p.data = view` for parameters, a `setattr` on the owning submodule for
    buffers."""
    named = list(named)
    flat = torch.empty(sum(t.numel() for _, t in named), dtype=torch.float32, device=named[0][1].device)
    for (name, t), view in zip(named, views(flat, named).values()):
        view.copy_(t.detach().float())
        assign(name, t, view)
    return flat


def views(flat: torch.Tensor, named: Named) -> Dict[str, torch.Tensor]:
    """name -> the slice of `flat` (a parameter arena, a gradient arena, an EMA shadow) with that tensor's place and shape."""
    out, off = {}, 0
    for name, t in named:
        n = t.numel()
        out[name] = flat[off:off + n].view(t.shape)
        off += n
    return out


def arena_of(tensors: List[torch.Tensor]) -> Optional[torch.Tensor]:
    """The flat fp32 tensor `tensors` are consecutive views of, if they are (same storage, back to back)."""
    if not tensors or any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        return None
    base = tensors[0]
    off = base.storage_offset()
    for t in tensors:
        if t.untyped_storage().data_ptr() != base.untyped_storage().data_ptr() or t.storage_offset() != off:
            return None
        off += t.numel()
    total = off - base.storage_offset()
    return torch.as_strided(base, (total,), (1,), base.storage_offset())


# ---- the one-tensor alias ------------------------------------------------------------------------------------------------
def flat_alias(module: nn.Module, flat: Optional[torch.Tensor] = None, create: bool = False) -> Optional[nn.Parameter]:
    """The leaf Parameter that aliases `module`'s whole arena (its `flat_parameter()`), or None when there is none and `create`
    is off.  It lives in `module.__dict__`, out of nn.Module's parameter registry: the per-tensor Parameters, `parameters()` and
    `state_dict()` stay what they were.  Given `flat`, an alias left on an earlier arena (the arena was rebuilt: `.to()`, new
    tensors loaded) is put on this one."""
    fp = module.__dict__.get("_flat_param")
    if fp is None:
        if create:
            fp = module.__dict__["_flat_param"] = nn.Parameter(flat, requires_grad=True)
    elif flat is not None and fp.data_ptr() != flat.data_ptr():
        fp.data = flat
    return fp


# ---- workspace slot, graph token, pool -----------------------------------------------------------------------------------
class Workspace:
    """One activation workspace; `busy` while an autograd graph that saved into it is alive.  `owner` counts the
    training-mode forwards that took it: only the graph that still owns it may release it (a stale token of an earlier
    graph, collected late, must not free a workspace a newer graph saved its activations in)."""

    def __init__(self, nbytes: int, device, zero_head: int = 0) -> None:
        # Zeroed once, at allocation, all of it.  The native passes ask that only of the head (`zero_head` bytes: include/resr.h), but
        # the weight-gradient reduction also looks at slab entries no launch of the pass has written (padding rows / columns, the bias
        # part of a job without a bias) when it decides whether a lifted pass overflowed (csrc/wgrad.hip, common.h grad_prescale): a
        # non-finite bit pattern that recycled memory happened to hold there set the sticky back-off of a workspace's FIRST pass, so
        # that pass and the next one differed by the lift -- depending on what the process had freed before.
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.busy = False
        self.owner = 0

    def acquire(self) -> int:
        self.owner += 1
        self.busy = True
        return self.owner

    def release(self, owner: int) -> None:
        if owner == self.owner:
            self.busy = False


class GraphToken:
    """Lifetime of one training-mode graph: takes the workspace and gives it back when the graph's backward has run
    (`finish()`) or when the graph is dropped without one -- once, whichever comes first.  `on_open` / `on_finish` run with
    the two ends (a module's count of live graphs)."""

    def __init__(self, ws: Workspace, on_open: Optional[Callable[[], None]] = None,
                 on_finish: Optional[Callable[[], None]] = None) -> None:
        self.ws, self.owner, self.open, self.on_finish = ws, ws.acquire(), True, on_finish
        if on_open is not None:
            on_open()

    def finish(self) -> None:
        if self.open:
            self.open = False
            if self.on_finish is not None:
                self.on_finish()
            self.ws.release(self.owner)

    def __del__(self) -> None:
        self.finish()


def take(pools: Dict[tuple, list], key: tuple, device, make: Callable[[], Workspace]) -> Workspace:
    """The first workspace of `pools[key]` that no live graph holds and that is on `device`, else a new one from `make()`."""
    pool = pools.setdefault(key, [])
    for ws in pool:
        if not ws.busy and ws.buf.device == device:
            return ws
    ws = make()
    pool.append(ws)
    return ws
