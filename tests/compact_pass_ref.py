"""Plain references of every pass of resr_compact_forward_train / resr_compact_backward (csrc/compact.hip, compact_train.hip), CPU only,
and the rule that judges the passes one by one on the values each was given (tests/test_gpu_compact_train_passes.py; this file's own
check is tests/test_compact_pass_ref.py).

Every function restates its pass from the DEFINITIONS in include/resr.h ("Compact generator", "Compact generator: training") and
include/resr_debug.h (the three element-wise kernels) on NCHW tensors; the convolutions are tests/conv_ref.py's.  Nothing here shares
index arithmetic with the kernels: a pixel shuffle is a reshape, a transposed convolution is conv_ref.conv3x3 on the transposed,
flipped weights.  float64 is the reference, float32 ON THE SAME INPUTS the yardstick the allowance A comes from (conv_ref.allowance).

Values.  A pass is judged on what the device pass READ: the stored x_in, z_k, a_k, g_t, g_z_k, g_xin, and the weights as handed to
resr_pack_weights (fast: their f16 rounding).  Fast mode is judged in the lifted domain, as stored: the backward pass runs on
g_y * lift (compact_grad_ref.lift_of) and only dW, db, dslope and gx leave times 1 / lift.

  judge_passes     the per-pass rule; `dev` holds what one forward + backward left (the GPU test reads it from the workspace through
                   resr_debug_compact_train_offsets, emulate_passes computes it on the CPU with the same roundings).
  emulate_passes   the CPU stand-in for the device, with an optional planted fault (FAULTS): the evidence that the rule rejects a
                   wrong pass.
  pinned_backward  the whole backward in float64 with masks and forward values taken from the arguments: one fixed linear map of g_y.
"""
import torch

from tests import compact_grad_ref as G
from tests import conv_ref as R

F64, F32 = torch.float64, torch.float32
F32_HALF_ULP = 2.0 ** -24 * 1.01    # half an fp32 ulp relative to the value, the slack of conv_ref.F16_HALF_ULP

# (num_conv, upscale, act, slopes, batch, (h, w), seed), compact_grad_ref.make_case's format.
# 3a: at most two activation layers, so nothing the backward writes is overwritten before it returns -- every pass is observable.
CASES_3A = [
    (1, 4, "prelu", "drawn", 2, (5, 7), 0),
    (0, 2, "prelu", "drawn", 1, (18, 33), 0),
    (1, 3, "leakyrelu", None, 1, (33, 17), 0),
    (1, 1, "relu", None, 2, (9, 40), 0),
]
# (case, power of two the cotangent is multiplied by): a dense randn cotangent (lift 16), one far below (a large lift), one with lift 1
RUNS_3A = [(c, 0) for c in CASES_3A] + [(CASES_3A[0], -14), (CASES_3A[3], 7)]
# 3b: the existing general cases of tests/test_gpu_compact_train.py, both parities of the ping-pong
CASES_3B = [
    (2, 4, "prelu", "drawn", 2, (5, 7), 0),
    (3, 2, "relu", None, 2, (18, 33), 0),
    (2, 1, "prelu", "drawn", 1, (37, 53), 0),
]
YARDSTICK_WORST = 2e-3    # 3b's condition on the reference alone: the pinned f16 emulation's worst tensor stays below this


def run_id(run):
    case, shift = run
    return G.case_id(case) + (f"-gy2^{shift}" if shift else "")


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def pixel_shuffle(t, s):
    """y[n,c,sY+i,sX+j] = t[n, c s^2 + i s + j, Y, X]."""
    n, c, h, w = t.shape
    return t.reshape(n, c // (s * s), s, s, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, c // (s * s), h * s, w * s)


def pixel_unshuffle(g, s):
    """The inverse (and, being a permutation, the adjoint): out[n, c s^2 + i s + j, Y, X] = g[n,c,sY+i,sX+j]."""
    n, c, hh, ww = g.shape
    return g.reshape(n, c, hh // s, s, ww // s, s).permute(0, 1, 3, 5, 2, 4).reshape(n, c * s * s, hh // s, ww // s)


def nearest(x, s):
    return x.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)


def residual_adjoint(gy, s, dtype):
    """sum_{i,j<s} gy[n,c,sY+i,sX+j], added in the order (i, j) to one accumulator (resr_debug_compact_residual_bwd)."""
    g = gy.to(dtype)
    acc = torch.zeros_like(g[:, :, ::s, ::s])
    for i in range(s):
        for j in range(s):
            acc = acc + g[:, :, i::s, j::s]
    return acc


def transposed(wt):
    """The weights of the backward-data pass of conv [cout,cin,3,3]: [cin,cout,3,3], taps flipped."""
    return wt.transpose(0, 1).flip(2, 3).contiguous()


def dgrad(g, wt, dtype):
    """g_in[n,c,y,x] = sum_{o,dy,dx} W[o,c,dy,dx] * g[n,o,y-dy+1,x-dx+1]: conv_ref.conv3x3 on the transposed, flipped weights."""
    return R.conv3x3(g, transposed(wt), dtype)[0]


def slope_table(sd, k, act_type):
    """The 64 fp32 slopes of activation layer k as the kernels read them: the PReLU parameters, 0.1f (LeakyReLU) or 0 (ReLU)."""
    if act_type == "prelu":
        return sd[f"body.{2 * k + 1}.weight"].detach().float().cpu()
    return torch.full((64,), 0.1 if act_type == "leakyrelu" else 0.0, dtype=F32)


def act_fwd(z, slopes, tdtype):
    """a = z > 0 ? z : slope[c] * z, evaluated in fp32 and rounded once to the storage type: defined bit for bit."""
    zf = z.float()
    return torch.where(zf > 0, zf, slopes.float().view(1, -1, 1, 1) * zf).to(tdtype)


def act_factor(z, slopes, dtype=F64):
    """m = z > 0 ? 1 : slope[c]."""
    return torch.where(z.to(dtype) > 0, torch.ones((), dtype=dtype), slopes.to(dtype).view(1, -1, 1, 1).expand(z.shape))


def weights_as_packed(sd, k, fast):
    """Conv k's weight as resr_pack_weights is handed it: the fp32 parameter, fast mode its f16 rounding."""
    w = sd[f"body.{2 * k}.weight"].detach().float().cpu()
    return w.half().float() if fast else w


def _bias(sd, k):
    return sd[f"body.{2 * k}.bias"].detach().float().cpu()


def _seq_sum32(terms):
    """[n,c,h,w] float32 -> [c]: one fp32 accumulator per channel, the pixels added one after the other."""
    t = terms.permute(1, 0, 2, 3).reshape(terms.shape[1], -1)
    acc = torch.zeros(t.shape[0], dtype=F32)
    for p in range(t.shape[1]):
        acc += t[:, p]
    return acc


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---- the per-pass rule ----------------------------------------------------------------------------------------------------------------
def judge_passes(dev, sd, x, gy, num_conv, upscale, act_type, fast):
    """One row per pass: {"pass", "kind", "ratio", "bad", "allowance", "worst", ...}; a pass is right when bad == 0.

    dev (CPU tensors, NCHW, in the storage type -- f16 fast, f32 strict -- unless noted):
      lift            the power of two the backward ran at (1.0: strict, or a cotangent that needs none)
      x_in [n,32,h,w], z / a: lists of [n,64,h,w] (k = 0 .. num_conv), t [n,3s^2,h,w] fp32, y fp32
      g_t [n,cpl,h,w], gz: list of g_z_k [n,64,h,w], g_xin [n,32,h,w]
      grads {parameter name: fp32}, gx [n,3,h,w] fp32
    kind "bits": the result is defined bit for bit, bad = the number of elements whose bits differ.  "zero": elements that must be
    exactly zero, bad = those that are not.  Else conv_ref.judge's kinds; A = conv_ref.allowance of the float32 evaluation.

    g_z_k.  The device computes st(st(g_a) * m) from the g_a the transposed convolution gives (st: the store's rounding; act_bwd runs
    in place, so g_a itself is not observable).  With |g_a - g_a64| <= A + hu |g_a64| (the convolution within its allowance, then the
    f16 store; strict: the fp32 result is the store, hu = 0) the product is within (A + hu |g_a64|) |m| of g_z64 = g_a64 m, and its
    own rounding adds half an ulp of the element (fast: at least the f16 subnormal spacing, as conv_ref.bound's "f16").
    dslope_k.  sum_pixels g_a min(z_k, 0) / lift: only pixels with z_k <= 0 contribute, each with g_a's error times |z_k|; the fp32
    sum itself gets A of the plain fp32 evaluation (one accumulator per channel, pixel after pixel)."""
    rows = []
    s, nb = upscale, num_conv + 1
    tdt = torch.float16 if fast else F32
    kind = "f16" if fast else "f32"
    hu_store = R.F16_HALF_ULP if fast else 0.0                      # g_a's store
    hu_prod = R.F16_HALF_ULP if fast else F32_HALF_ULP              # the rounding of g_a * m
    floor = R.F16_SUBNORMAL if fast else 2.0 ** -149                # the subnormal spacing of the storage type
    lift = float(dev["lift"])
    inv = 1.0 / lift
    n, _, h, w = x.shape
    c_t = 3 * s * s
    W = [weights_as_packed(sd, k, fast) for k in range(nb + 1)]
    sl = [slope_table(sd, k, act_type) for k in range(nb)]
    xf, gyf = x.detach().float().cpu(), gy.detach().float().cpu()

    def bits(name, got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        differ = _bits(got) != _bits(want)
        worst = int(differ.reshape(-1).to(torch.uint8).argmax())
        rows.append({"pass": name, "kind": "bits", "bad": int(differ.sum()), "ratio": float(differ.any()), "allowance": 0.0, "worst": worst,
                     "got": float(got.reshape(-1)[worst]), "want": float(want.reshape(-1)[worst])})

    def zero(name, got):
        nz = got != 0
        worst = int(nz.reshape(-1).to(torch.uint8).argmax()) if nz.numel() else 0
        rows.append({"pass": name, "kind": "zero", "bad": int(nz.sum()), "ratio": float(nz.any()), "allowance": 0.0, "worst": worst,
                     "got": float(got.reshape(-1)[worst]) if nz.numel() else 0.0, "want": 0.0})

    def num(name, got, r64, r32, k, extra=None, allowance=None):
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        rec = R.judge(got, r64, r32, k, extra)
        rows.append({"pass": name, "kind": k, "bad": rec["bad"], "ratio": rec["ratio"], "allowance": rec["allowance"] if allowance is None else allowance,
                     "worst": rec["worst"], "got": rec["got"], "want": rec["want"], "kernel_err": rec["kernel_err"], "cpu32_err": rec["cpu32_err"]})

    # ---- forward ----
    want = torch.zeros(n, 32, h, w, dtype=tdt)
    want[:, :3] = xf.to(tdt)
    bits("x_in", dev["x_in"], want)
    inp = dev["x_in"][:, :3]
    for k in range(nb):
        b = _bias(sd, k)
        num(f"z_{k}", dev["z"][k], R.conv3x3(inp, W[k], F64, bias=b)[0], R.conv3x3(inp, W[k], F32, bias=b)[0], kind)
        bits(f"a_{k}", dev["a"][k], act_fwd(dev["z"][k], sl[k], tdt))
        inp = dev["a"][k]
    b = _bias(sd, nb)
    num("t", dev["t"], R.conv3x3(inp, W[nb], F64, bias=b)[0], R.conv3x3(inp, W[nb], F32, bias=b)[0], "f32")
    bits("y", dev["y"], pixel_shuffle(dev["t"].float(), s) + nearest(xf, s))

    # ---- backward ----
    want = torch.zeros_like(dev["g_t"])
    want[:, :c_t] = (pixel_unshuffle(gyf, s) * torch.tensor(lift, dtype=F32)).to(tdt)
    bits("g_t", dev["g_t"], want)
    zero("g_t_pad", dev["g_t"][:, c_t:])
    g = dev["g_t"][:, :c_t]
    last = 2 * nb
    dw64, db64 = R.wgrad(inp, g, inv, F64)
    dw32, db32 = R.wgrad(inp, g, inv, F32)
    num(f"dW_{nb}", dev["grads"][f"body.{last}.weight"], dw64, dw32, "f32")
    num(f"db_{nb}", dev["grads"][f"body.{last}.bias"], db64, db32, "f32")
    for k in range(nb - 1, -1, -1):
        ga64, ga32 = dgrad(g, W[k + 1], F64), dgrad(g, W[k + 1], F32)
        a_ga, _ = R.allowance(ga64, ga32)
        zk = dev["z"][k]
        m = act_factor(zk, sl[k])
        gz64 = ga64 * m
        ga_err = a_ga + hu_store * ga64.abs()
        bound = ga_err * m.abs() + torch.clamp(hu_prod * gz64.abs(), min=floor)
        num(f"g_z_{k}", dev["gz"][k], gz64, None, "f32", extra=bound, allowance=a_ga)
        if act_type == "relu":
            zero(f"g_z_{k}_where_z<=0", dev["gz"][k][zk <= 0])
        if act_type == "prelu":
            zneg = torch.clamp(zk.double(), max=0.0)
            ds64 = (ga64 * zneg).sum(dim=(0, 2, 3)) * inv
            ds32 = _seq_sum32(ga32 * zneg.float()) * torch.tensor(inv, dtype=F32)
            num(f"dslope_{k}", dev["grads"][f"body.{2 * k + 1}.weight"], ds64, ds32, "f32", extra=(ga_err * zneg.abs()).sum(dim=(0, 2, 3)) * inv)
        xk = dev["a"][k - 1] if k > 0 else dev["x_in"][:, :3]
        g = dev["gz"][k]
        dw64, db64 = R.wgrad(xk, g, inv, F64)
        dw32, db32 = R.wgrad(xk, g, inv, F32)
        num(f"dW_{k}", dev["grads"][f"body.{2 * k}.weight"], dw64, dw32, "f32")
        num(f"db_{k}", dev["grads"][f"body.{2 * k}.bias"], db64, db32, "f32")
    num("g_xin", dev["g_xin"][:, :3], dgrad(g, W[0], F64), dgrad(g, W[0], F32), kind)
    zero("g_xin_pad", dev["g_xin"][:, 3:])
    v = dev["g_xin"][:, :3]
    num("gx", dev["gx"], v.double() * inv + residual_adjoint(gyf, s, F64), v.float() * torch.tensor(inv, dtype=F32) + residual_adjoint(gyf, s, F32), "f32")
    return rows


def bad_passes(rows):
    return {r["pass"]: r["bad"] for r in rows if r["bad"]}


# ---- the CPU stand-in for the device ---------------------------------------------------------------------------------------------------
# planted faults of emulate_passes; each is wrong in ONE pass
FAULTS = ("dgrad_drops_border_column", "mask_from_a", "g_t_pad_nonzero", "dslope_reads_other_z", "db_without_unlift", "ping_pong_swapped")


def emulate_passes(sd, x, gy, num_conv, upscale, act_type, fast=True, fault=None):
    """What one forward + backward leaves, computed in float64 and rounded wherever the native pass stores (`dev` of judge_passes, with
    g_z of every layer).  fault: None, one of FAULTS, or (one of FAULTS, at) to say where --
      dgrad_drops_border_column  the backward-data pass of convolution `at` (default: the last; 0: the one that writes g_xin) leaves the
                                 last column of its result zero
      mask_from_a                act_bwd of layer `at` (default: the top one) takes its mask from a_k > 0 (wrong where the slope is negative)
      g_t_pad_nonzero            one pad channel of g_t holds a value in one pixel
      dslope_reads_other_z       the slope gradient of layer `at` (default: the top one) reads z_{k-1}
      db_without_unlift          db of conv 0 leaves without the 1 / lift
      ping_pong_swapped          dW, db of conv 0 read the other gradient buffer (g_z of layer 1)"""
    fault, at = fault if isinstance(fault, tuple) else (fault, None)
    assert fault is None or fault in FAULTS, fault
    s, nb = upscale, num_conv + 1
    tdt = torch.float16 if fast else F32
    xf, gyf = x.detach().float().cpu(), gy.detach().float().cpu()
    n, _, h, w = xf.shape
    c_t, cpl = 3 * s * s, (3 * s * s + 31) // 32 * 32
    W = [weights_as_packed(sd, k, fast) for k in range(nb + 1)]
    sl = [slope_table(sd, k, act_type) for k in range(nb)]
    x_in = torch.zeros(n, 32, h, w, dtype=tdt)
    x_in[:, :3] = xf.to(tdt)
    z, a = [], []
    inp = x_in[:, :3]
    for k in range(nb):
        z.append(R.conv3x3(inp, W[k], F64, bias=_bias(sd, k))[0].to(tdt))
        a.append(act_fwd(z[k], sl[k], tdt))
        inp = a[k]
    t = R.conv3x3(inp, W[nb], F64, bias=_bias(sd, nb))[0].float()
    y = pixel_shuffle(t, s) + nearest(xf, s)
    lift = G.lift_of(gyf) if fast else 1.0
    inv = 1.0 / lift
    g_t = torch.zeros(n, cpl, h, w, dtype=tdt)
    g_t[:, :c_t] = (pixel_unshuffle(gyf, s) * torch.tensor(lift, dtype=F32)).to(tdt)
    if fault == "g_t_pad_nonzero":
        g_t[0, c_t, h // 2, w // 2] = 1.0
    grads = {}
    g = g_t[:, :c_t]
    dw, db = R.wgrad(inp, g, inv, F64)
    grads[f"body.{2 * nb}.weight"], grads[f"body.{2 * nb}.bias"] = dw.float(), db.float()
    gz = [None] * nb
    for k in range(nb - 1, -1, -1):
        ga = dgrad(g, W[k + 1], F64).to(tdt)
        top = k == (nb - 1 if at is None else at)                          # the layer a fault of an activation layer sits in
        if fault == "dgrad_drops_border_column" and k + 1 == (nb if at is None else at):
            ga[..., -1] = 0
        m = act_factor(a[k] if fault == "mask_from_a" and top else z[k], sl[k], F32)
        gz[k] = (ga.float() * m).to(tdt)                                   # one fp32 product, rounded once
        if act_type == "prelu":
            zsrc = z[k - 1] if fault == "dslope_reads_other_z" and top else z[k]
            grads[f"body.{2 * k + 1}.weight"] = ((ga.double() * torch.clamp(zsrc.double(), max=0.0)).sum(dim=(0, 2, 3)) * inv).float()
        xk = a[k - 1] if k > 0 else x_in[:, :3]
        gk = gz[1] if fault == "ping_pong_swapped" and k == 0 else gz[k]
        dw, db = R.wgrad(xk, gk, inv, F64)
        if fault == "db_without_unlift" and k == 0:
            db = db * lift
        grads[f"body.{2 * k}.weight"], grads[f"body.{2 * k}.bias"] = dw.float(), db.float()
        g = gz[k]
    g_xin = torch.zeros(n, 32, h, w, dtype=tdt)
    g_xin[:, :3] = dgrad(g, W[0], F64).to(tdt)
    if fault == "dgrad_drops_border_column" and at == 0:
        g_xin[..., -1] = 0
    gx = g_xin[:, :3].float() * torch.tensor(inv, dtype=F32) + residual_adjoint(gyf, s, F32)
    return {"lift": lift, "x_in": x_in, "z": z, "a": a, "t": t, "y": y, "g_t": g_t, "gz": gz, "g_xin": g_xin, "grads": grads, "gx": gx}


def device_grads(dev):
    """{name: gradient} with "x", the shape compact_grad_ref.errors takes."""
    out = dict(dev["grads"])
    out["x"] = dev["gx"]
    return out


# ---- end to end, masks pinned ----------------------------------------------------------------------------------------------------------
def forward64(sd, x, num_conv, act_type):
    """(x_in, [z_k], [a_k]) of the float64 forward on the state dict's own (unrounded) values."""
    xi = x.detach().double().cpu()
    z, a = [], []
    inp = xi
    for k in range(num_conv + 1):
        z.append(R.conv3x3(inp, sd[f"body.{2 * k}.weight"].detach().double().cpu(), F64, bias=sd[f"body.{2 * k}.bias"].detach().cpu())[0])
        a.append(act_factor(z[k], _slopes64(sd, k, act_type)) * z[k])
        inp = a[k]
    return xi, z, a


def _slopes64(sd, k, act_type):
    """The slopes as float64 autograd of the upstream module takes them (LeakyReLU: the double 0.1, not the kernels' 0.1f -- 1.5e-9 apart)."""
    if act_type == "prelu":
        return sd[f"body.{2 * k + 1}.weight"].detach().double().cpu()
    return torch.full((64,), 0.1 if act_type == "leakyrelu" else 0.0, dtype=F64)


def pinned_backward(sd, x_in, z, a, gy, num_conv, upscale, act_type, round16=False, lift=None):
    """{name: gradient} with "x": the whole backward in float64, the masks (z_k > 0) and the forward values (x_in [n,3,h,w], z_k, a_k:
    weight gradients read a_{k-1}, slope gradients z_k) taken from the arguments -- for fixed arguments one linear map of g_y.  The
    weights are `sd`'s as given.  round16: g_t, every g_a and every g_z are rounded to f16 at `lift` (default: compact_grad_ref.lift_of
    of g_y), as compact_grad_ref.evaluate("emu16") rounds them, and the backward-data passes run on the f16 rounding of the weights,
    which is what fast mode packs; sums stay exact."""
    s, nb = upscale, num_conv + 1
    g_y = gy.detach().double().cpu()
    lift = (G.lift_of(g_y) if round16 else 1.0) if lift is None else float(lift)
    rb = (lambda v: v.half().double()) if round16 else (lambda v: v)
    wt = lambda k: (lambda v: v.half().double() if round16 else v)(sd[f"body.{2 * k}.weight"].detach().double().cpu())
    x_in = x_in.double()
    grads = {}
    g = rb(pixel_unshuffle(g_y, s) * lift)
    dw, db = R.wgrad(a[nb - 1], g, 1.0, F64)
    grads[f"body.{2 * nb}.weight"], grads[f"body.{2 * nb}.bias"] = dw / lift, db / lift
    for k in range(nb - 1, -1, -1):
        ga = rb(dgrad(g, wt(k + 1), F64))
        zk = z[k].double()
        slopes = _slopes64(sd, k, act_type)
        if act_type == "prelu":
            grads[f"body.{2 * k + 1}.weight"] = (ga * torch.clamp(zk, max=0.0)).sum(dim=(0, 2, 3)) / lift
        g = rb(ga * act_factor(zk, slopes))
        dw, db = R.wgrad(a[k - 1] if k > 0 else x_in, g, 1.0, F64)
        grads[f"body.{2 * k}.weight"], grads[f"body.{2 * k}.bias"] = dw / lift, db / lift
    grads["x"] = dgrad(g, wt(0), F64) / lift + residual_adjoint(g_y, s, F64)
    return {k: grads[k] for k in list(sd) + ["x"]}


def pinned_gate(grads, sd, dev, gy, num_conv, upscale, act_type):
    """Section 3b, fast mode: `grads` ({name: gradient} with "x") against the float64 backward pinned on dev's x_in, z_k, a_k and run on the
    weights fast mode packs (their f16 rounding: the linear map the device evaluates), next to the yardstick -- the same map with the
    f16 roundings of the gradients.  Returns the record; "ok" says worst and median are within 2 x the yardstick's, "condition" that the
    yardstick's own worst tensor is below YARDSTICK_WORST."""
    packed = {k: (v.detach().float().cpu().half().float() if v.dim() == 4 else v.detach().float().cpu()) for k, v in sd.items()}
    args = (dev["x_in"][:, :3], dev["z"], dev["a"], gy, num_conv, upscale, act_type)
    g64p = pinned_backward(packed, *args, round16=False)
    e16p = pinned_backward(packed, *args, round16=True)
    errs, yard = G.errors(grads, g64p), G.errors(e16p, g64p)
    worst, median = G.worst_median(errs)
    y_worst, y_median = G.worst_median(yard)
    return {"worst": worst, "median": median, "yardstick_worst": y_worst, "yardstick_median": y_median, "worst_tensor": max(errs, key=errs.get),
            "condition": y_worst < YARDSTICK_WORST, "ok": worst <= 2.0 * y_worst and median <= 2.0 * y_median}
