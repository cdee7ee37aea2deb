"""CPU: the flat arena, its one-tensor alias and the workspace lifetime that `Generator`, `Discriminator` and `SRVGGNetCompact`
share (real_esrgan-pytorch_amd/_arena.py).  The first group goes through the modules' public surface only; the second is on the
helpers themselves.  The native calls involved are host-side planning: no GPU."""
import gc

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


# ---- through the public surface ------------------------------------------------------------------------------------------
# name -> (constructor, the method listing the arena's tensors, the method returning the arena)
ARENAS = {
    "generator": (lambda R: R.Generator(3, 3, 2, n_blocks=1), "named_parameters", "flat_parameters"),
    "discriminator": (lambda R: R.Discriminator(), "named_parameters", "flat_parameters"),
    "discriminator_uv": (lambda R: R.Discriminator(), "named_buffers", "flat_uv"),
    "compact": (lambda R: R.SRVGGNetCompact(num_conv=2), "named_parameters", "flat_parameters"),
}


def _arena_case(R, which):
    make, named, flat = ARENAS[which]
    torch.manual_seed(1)
    m = make(R)
    return m, (lambda: list(getattr(m, named)())), getattr(m, flat)


def _assert_views(flat, named):
    assert flat.dtype == torch.float32 and flat.dim() == 1
    assert flat.numel() == sum(t.numel() for _, t in named)
    off = 0
    for name, t in named:
        assert t.dtype == torch.float32 and t.data_ptr() == flat.data_ptr() + 4 * off, name
        off += t.numel()
    assert torch.equal(flat, torch.cat([t.detach().reshape(-1) for _, t in named]))


@pytest.mark.parametrize("which", sorted(ARENAS))
def test_arena_views_roundtrip_and_identity(built, which):
    m, named, flat_of = _arena_case(built, which)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    values = {k: t.detach().clone() for k, t in named()}
    flat = flat_of()
    _assert_views(flat, named())                                   # views back to back, total size
    assert list(m.state_dict()) == list(before)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                        # state_dict equal before and after
    for k, t in named():
        assert torch.equal(t.detach(), values[k]), k
    assert flat_of() is flat                                       # the same object on a second call
    m.load_state_dict({k: v + 1 for k, v in before.items()})
    assert flat_of() is flat                                       # ... and a load is seen through it, without a rebuild
    assert torch.equal(flat, torch.cat([values[k].reshape(-1) + 1 for k, _ in named()]))


@pytest.mark.parametrize("trigger", ["data_replaced", "double_float"])
@pytest.mark.parametrize("which", sorted(ARENAS))
def test_arena_is_rebuilt_when_a_tensor_left_it(built, which, trigger):
    m, named, flat_of = _arena_case(built, which)
    flat = flat_of()
    kept = flat.clone()
    if trigger == "data_replaced":
        t = named()[1][1]
        t.data = t.data.clone()
    else:
        m.double().float()
    new = flat_of()
    assert new is not flat and new.data_ptr() != flat.data_ptr()
    assert torch.equal(new, kept)
    _assert_views(new, named())
    assert flat_of() is new


@pytest.mark.parametrize("which", ["generator", "discriminator"])
def test_flat_parameter_alias_follows_the_arena(built, which):
    m, named, flat_of = _arena_case(built, which)
    fp = m.flat_parameter()
    assert isinstance(fp, torch.nn.Parameter) and fp.requires_grad and fp.is_leaf
    assert fp.data_ptr() == flat_of().data_ptr() and fp.numel() == flat_of().numel()
    assert m.flat_parameter() is fp
    assert all(p is not fp for p in m.parameters())                # not one of the module's parameters
    keys = list(m.state_dict())
    t = named()[0][1]
    t.data = t.data.clone()                                        # the arena is rebuilt at the next call
    assert m.flat_parameter() is fp
    assert fp.data_ptr() == flat_of().data_ptr()
    assert list(m.state_dict()) == keys


def test_discriminator_alias_mirrors_requires_grad_and_zero_grad(built):
    d = built.Discriminator()
    fp = d.flat_parameter()
    d.requires_grad_(False)
    assert not fp.requires_grad and not any(p.requires_grad for p in d.parameters())
    d.requires_grad_(True)
    assert fp.requires_grad
    fp.grad = torch.ones_like(fp)
    assert d.flat_grad() is fp.grad
    grad = fp.grad
    d.zero_grad(set_to_none=False)
    assert fp.grad is grad and not fp.grad.any()
    fp.grad = torch.ones_like(fp)
    d.zero_grad()
    assert fp.grad is None and d.flat_grad() is None


def test_generator_zero_grad_leaves_the_alias_alone(built):
    g = built.Generator(3, 3, 2, n_blocks=1)
    fp = g.flat_parameter()
    grad = torch.ones_like(fp)
    fp.grad = grad
    g.zero_grad()
    assert fp.grad is grad and bool(fp.grad.all())
    g.zero_grad(set_to_none=False)
    assert fp.grad is grad and bool(fp.grad.all())


# ---- the helpers themselves ----------------------------------------------------------------------------------------------
@pytest.fixture()
def A():
    import real_esrgan_pytorch_amd._arena as _arena
    return _arena


def _three(flat):
    return [flat[0:6].view(2, 3), flat[6:10], flat[10:12].view(2, 1)]


def test_is_arena(A):
    flat = torch.arange(12, dtype=torch.float32)
    a, b, c = _three(flat)
    assert A.is_arena(flat, [a, b, c])
    assert not A.is_arena(None, [a, b, c])
    assert not A.is_arena(flat, [a, flat[7:10], c])                          # a gap
    assert not A.is_arena(flat, [a, flat[6:9], flat[10:12]])                 # a gap behind a short member
    assert not A.is_arena(flat, [b, a, c])                                   # a swapped pair
    assert not A.is_arena(flat, [a, b.clone(), c])                           # a member with memory of its own
    longer = torch.arange(14, dtype=torch.float32)
    assert not A.is_arena(longer, _three(longer))                            # trailing elements
    assert not A.is_arena(flat, [a, b])                                      # ... however they arise
    half = torch.zeros(24, dtype=torch.float16)                              # a non-fp32 member at the right address
    as32 = half.view(torch.float32)
    assert A.is_arena(as32, [as32[0:6], as32[6:12]])
    assert not A.is_arena(as32, [as32[0:6], half[12:24]])
    assert not A.is_arena(flat.double(), _three(flat.double()))


def test_build_and_views(A):
    src = {"w": torch.randn(2, 3, dtype=torch.float64), "b": torch.randn(4), "s": torch.randn(2, 1).t()}
    out = {}
    flat = A.build(src.items(), lambda name, t, view: out.__setitem__(name, view))
    assert flat.dtype == torch.float32 and flat.numel() == 12
    assert A.is_arena(flat, out.values()) and list(out) == list(src)
    for k, t in src.items():
        assert out[k].shape == t.shape and torch.equal(out[k], t.float()), k
    v = A.views(flat, src.items())
    assert list(v) == list(src)
    for k in src:
        assert v[k].data_ptr() == out[k].data_ptr() and v[k].shape == src[k].shape
    assert A.arena_of(list(out.values())).data_ptr() == flat.data_ptr()
    assert A.arena_of([out["w"], out["s"]]) is None


def test_take_reuses_free_slots_per_device(A):
    made = []

    def make(device="cpu"):
        made.append(A.Workspace(64, device, 16))
        return made[-1]
    pools, cpu = {}, torch.device("cpu")
    a = A.take(pools, ("k",), cpu, make)
    assert len(made) == 1 and not a.busy and not a.buf[:16].any()
    assert A.take(pools, ("k",), cpu, make) is a and len(made) == 1          # a free slot is reused
    owner = a.acquire()
    b = A.take(pools, ("k",), cpu, make)
    assert b is not a and len(made) == 2 and pools[("k",)] == [a, b]         # a busy slot gives a second one
    a.release(owner)
    assert A.take(pools, ("k",), cpu, make) is a and len(made) == 2
    assert A.take(pools, ("other",), cpu, make) not in (a, b) and len(made) == 3
    elsewhere = {("k",): [A.Workspace(64, "meta")]}                          # a free slot on another device is skipped
    c = A.take(elsewhere, ("k",), cpu, make)
    assert c.buf.device == cpu and len(made) == 4 and len(elsewhere[("k",)]) == 2


def test_stale_owner_does_not_release(A):
    ws = A.Workspace(8, "cpu")
    first = ws.acquire()
    ws.release(first)
    second = ws.acquire()
    assert second != first and ws.busy
    ws.release(first)                                                        # the earlier graph's number, collected late
    assert ws.busy
    ws.release(second)
    assert not ws.busy


def test_token_finishes_once_and_on_drop(A):
    ws, log = A.Workspace(8, "cpu"), []
    tok = A.GraphToken(ws, lambda: log.append("open"), lambda: log.append("finish"))
    assert ws.busy and log == ["open"]
    tok.finish()
    assert not ws.busy and log == ["open", "finish"]
    newer = A.GraphToken(ws)
    tok.finish()                                                             # twice: releases once, fires the callback once
    del tok
    gc.collect()
    assert ws.busy and log == ["open", "finish"]                            # ... and never the newer graph's slot
    del newer                                                                # dropped without a backward: released
    gc.collect()
    assert not ws.busy
    dropped = A.GraphToken(ws, None, lambda: log.append("finish"))
    del dropped
    gc.collect()
    assert not ws.busy and log == ["open", "finish", "finish"]
