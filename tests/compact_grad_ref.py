"""In-test references for the gradients of the compact generator (SRVGGNetCompact): three CPU evaluators of the output and of
every gradient (all parameters, and x) for a state dict, an input and a cotangent.

  f64    float64 autograd of upstream's module as tests/compact_oracle.py restates it: the oracle.
  f32    the same in float32.
  emu16  the f64 pass with straight-through f16 roundings exactly where fast mode stores 16-bit values.  Forward: x on its way into
         the first conv (the residual reads the fp32 x), the conv weights (not biases, not slopes), every pre-activation z_k, and every
         activation a_k, computed from the rounded z_k.  Backward: g_t (the gradient of the last conv's output), every g_a and every
         g_z, each rounded at the power-of-two lift the native pass works at (max |g_y| 2^k in [2^6, 2^7) when max |g_y| < 2^6).  Sums
         stay exact (float64).

`error(g, g64)` is the tests' distance: max |g - g64| / max |g64|.
"""
import math

import torch
import torch.nn.functional as F

from tests.compact_oracle import UpstreamCompact

# (num_conv, upscale, act, slopes, batch, (h, w), seed): the cases of tests/test_gpu_compact_train.py.  slopes: "drawn" = PReLU slopes in
# [-0.5, 1.5) as tests/test_gpu_compact.py draws them (negative, near zero and above 1), "identity" = every PReLU slope 1.0 (the net is
# linear: no mask can flip, the slope gradients still read z), None = the activation has none.  Between them: both cout_pad of the last
# conv (32: s = 1, 2, 3; 64: s = 4), sizes below one tile and across tile edges.
CASES = [
    (2, 4, "prelu", "drawn", 2, (5, 7), 0),
    (2, 3, "leakyrelu", None, 1, (37, 53), 0),
    (3, 2, "relu", None, 2, (18, 33), 0),
    (2, 1, "prelu", "drawn", 1, (37, 53), 0),
    (2, 4, "prelu", "identity", 2, (5, 7), 0),
    (2, 3, "prelu", "identity", 1, (37, 53), 0),
]


def case_id(case):
    nc, s, act, slopes, n, (h, w), _ = case
    return f"{nc}-x{s}-{act}{'-' + slopes if slopes else ''}-{n}x{h}x{w}"


def make_case(case):
    """(state dict, x, gy) of a case, fp32 on the CPU, from fixed seeds: upstream's init, x uniform in [0, 1), a dense randn cotangent."""
    nc, s, act, slopes, n, (h, w), seed = case
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in UpstreamCompact(nc, s, act).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():
        if v.dim() == 1 and int(k.split(".")[1]) % 2 == 1:   # PReLU slopes
            if slopes == "drawn":
                v.copy_(torch.rand(v.shape, generator=g) * 2 - 0.5)
            elif slopes == "identity":
                v.fill_(1.0)
    gen = torch.Generator().manual_seed(1000 + seed + h * w + n)
    x = torch.rand(n, 3, h, w, generator=gen)
    gy = torch.randn(n, 3, h * s, w * s, generator=gen)
    return sd, x, gy


def _f16(v):
    return v.to(torch.float16).to(v.dtype)


class _RoundFwd(torch.autograd.Function):
    """f16 rounding of the value, identity for the gradient."""

    @staticmethod
    def forward(ctx, v):
        return _f16(v)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    """Identity for the value; the gradient is rounded to f16 at `lift` (a power of two)."""

    @staticmethod
    def forward(ctx, v, lift):
        ctx.lift = lift
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return _f16(g * ctx.lift) / ctx.lift, None


def lift_of(gy):
    """The native pass's power-of-two lift for this cotangent: 2^k with max |g_y| 2^k in [2^6, 2^7) when max |g_y| < 2^6, else 1."""
    m = float(gy.abs().max()) * 2.0 ** -6
    if not (0.0 < m < 1.0) or not math.isfinite(m):
        return 1.0
    return 2.0 ** -math.floor(math.log2(m))


def _act(z, sd, k, act_type):
    if act_type == "prelu":
        return F.prelu(z, sd[f"body.{2 * k + 1}.weight"])
    if act_type == "leakyrelu":
        return F.leaky_relu(z, 0.1)
    return F.relu(z)


def evaluate(kind, sd, x, gy, num_conv, upscale, act_type):
    """kind "f64" | "f32" | "emu16" -> (y, {name: gradient}) with the state dict's parameter names and "x"; everything float64."""
    dtype = torch.float32 if kind == "f32" else torch.float64
    emu = kind == "emu16"
    p = {k: v.detach().to(dtype).cpu().clone().requires_grad_(True) for k, v in sd.items()}
    xi = x.detach().to(dtype).cpu().clone().requires_grad_(True)
    g = gy.detach().to(dtype).cpu()
    lift = lift_of(g) if emu else 1.0
    rf = _RoundFwd.apply if emu else (lambda v: v)
    rb = (lambda v: _RoundBwd.apply(v, lift)) if emu else (lambda v: v)
    h = rf(xi)
    for k in range(num_conv + 1):
        z = rb(rf(F.conv2d(h, rf(p[f"body.{2 * k}.weight"]), p[f"body.{2 * k}.bias"], padding=1)))     # z_k stored; g_z rounded
        h = rb(rf(_act(z, p, k, act_type)))                                                    # a_k stored; g_a rounded
    last = 2 * (num_conv + 1)
    t = rb(F.conv2d(h, rf(p[f"body.{last}.weight"]), p[f"body.{last}.bias"], padding=1))              # fp32 output; g_t rounded
    y = F.pixel_shuffle(t, upscale) + F.interpolate(xi, scale_factor=upscale, mode="nearest")
    names = list(p)
    grads = torch.autograd.grad(y, [p[n] for n in names] + [xi], g)
    out = {n: v.double() for n, v in zip(names, grads[:-1])}
    out["x"] = grads[-1].double()
    return y.detach().double(), out


def error(g, g64):
    return ((g.double().cpu() - g64).abs().max() / g64.abs().max()).item()


def errors(grads, grads64):
    """{name: error} over the tensors of grads64."""
    return {n: error(grads[n], g64) for n, g64 in grads64.items()}


def worst_median(errs):
    v = sorted(errs.values())
    n = len(v)
    return v[-1], (v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2]))
