"""Plain references of every pass of resr_generator_forward (training = 1) / resr_generator_backward (csrc/generator.hip), CPU only, and
the rule that judges the passes one by one on the values each was given (tests/test_gpu_generator_passes.py; this file's own check is
tests/test_generator_pass_ref.py).

Every function restates its pass from the DEFINITIONS in include/resr.h (ResrConvDesc: v = conv + bias, then mask / lrelu / res0 / res1 /
clamp; ResrWgradDesc; the sign words; the layout helpers) and the model (oracle/model_ref.py is the arithmetic) on NCHW tensors; the
convolutions are tests/conv_ref.py's, the layout, pool and add passes tests/layout_ref.py's.  Nothing here shares index arithmetic with the
kernels or with generator_pack_table: a chunk-planar tensor reaches this file already concatenated to [N,C,h,w], a transposed convolution
is conv_ref.conv3x3 on the transposed, flipped weights, and a mirrored dense-block pass is stated from the mathematics,
    g_o_k = m_k (.) sum_{j > k} W_j[:, 64 + 32 (k - 1) : 64 + 32 k]^T * g_o_j,   g_o_5 := gin through fold W_5,     k = 4 .. 1,
    g_x   = sum_{j = 1..5} W_j[:, 0:64]^T * g_o_j + t0 gin [+ e],
as one convolution over the channel concatenation [gin | g_o_4 | .. | g_o_{k+1}] with the weight slices concatenated the same way.
float64 is the reference, float32 ON THE SAME INPUTS the yardstick the allowance A comes from (conv_ref.allowance).

Values.  A pass is judged on what the device pass READ: the stored tensors of the workspace, the sign words as stored, the weights as
handed to resr_pack_weights -- fast mode their f16 rounding, the conv5 slices of the mirrored passes the f16 rounding of the fp32 product
fold * w (layout_ref.chunk_weights' rule: one fp32 product, then the conversion).  Fast mode is judged in the lifted domain, as stored:
the backward pass runs on g_y * lift and only dW, db and gx leave times 1 / lift.  Scalars are the descriptors' float32 constants, widened
(DEVICE below): the slope 0.2f, conv5's s0 = 0.2f, the packed fold 0.2f * 0.2f (an fp32 product), the weight gradient's scale 0.04f.

Composed roundings.  compact_pass_ref has to bound g_z = st(st(g_a) * m) because act_bwd runs in place.  Here no such pass exists: every
store of the generator's passes is ONE rounding of an fp32 epilogue value (mask, LeakyReLU and the residual terms are applied to the
accumulator before the store; a pool sums stored values in fp32 and rounds once), and every stored tensor a later pass reads is
observable -- gA, the only buffer written three times, through RESR_DEBUG_STOP = 1, 2, 3, and gT3 before its add_inplace through stop 4.
So every row is conv_ref.judge's plain bound (A, plus half an ulp of the element for an f16 store), or bits.  One term comes on top, in
fast mode's mirrored passes alone: resr_pack_weights may round fold * w to f16 once or twice (packed_weights has the two evaluations and
where they were met); the reference takes one and the bound of g_o_k and g_x carries sum |g| |W_other - W| -- one f16 ulp of a weight
of 1e-4 on about one element in 2^13, 1.1e-6 at most over every run of the GPU test, nothing in strict mode.

  judge_passes     the per-pass rule; `dev` holds what one forward + backward (and the four stopped runs) left.
  emulate_passes   the CPU stand-in for the device, with an optional planted fault (FAULTS): the evidence that the rule rejects a
                   wrong pass.
  pinned_backward  the whole backward in float64 with masks and forward values taken from the arguments: one fixed linear map of g_y.
  pinned_gate      section 3b: the device's gradients against that map, next to the same map with fast mode's f16 stores.
"""
import numpy as np
import torch

from tests import conv_ref as R
from tests import layout_ref as Y

F64, F32, F16 = torch.float64, torch.float32, torch.float16

# (upscale, N, h, w at the input, n_blocks, seed)
CASES_3A = [(4, 2, 5, 7, 1, 11), (4, 1, 9, 33, 1, 11), (2, 1, 10, 18, 1, 11), (1, 2, 12, 20, 1, 11)]
# (case, power of two the cotangent is multiplied by): a dense randn cotangent (lift 16 or 32), one far below (a large lift), one with lift 1
RUNS_3A = [(c, 0) for c in CASES_3A] + [(CASES_3A[0], -14), (CASES_3A[2], 7)]
CASES_3B = [(4, 2, 5, 7, 2, 11), (4, 1, 9, 33, 2, 11)]
YARDSTICK_WORST = 5e-3    # 3b's condition on the reference alone (the gate tests/test_gpu_mx.py sets for an f16 backward behind exact masks)
PRESCALE_LOG2 = 6         # csrc/generator.hip: the lift aims max |g_y| at [2^6, 2^7)


def case_id(case):
    s, n, h, w, nb, seed = case
    return f"x{s}-{n}x{h}x{w}-b{nb}"


def run_id(run):
    case, shift = run
    return case_id(case) + (f"-gy2^{shift}" if shift else "")


def make_case(case):
    """(sd, x, gy): tests/test_gpu_generator._setup's weights (conv4.bias + 0.5), a dense cotangent, and a uniform image of amplitude 32
    around 0.5: at these depths a unit-range image leaves every output within 0.38 .. 0.61, and ymask must hold both values."""
    from oracle import model_ref as M
    s, n, h, w, nb, seed = case
    sd = M.init_generator_state(seed, 3, 3, s, bias_noise=0.02)
    sd = {k: v for k, v in sd.items() if not k.startswith("trunk.") or int(k.split(".")[1]) < nb}
    sd["conv4.bias"] = sd["conv4.bias"] + 0.5
    gen = torch.Generator().manual_seed(5 + seed)
    return sd, (torch.rand(n, 3, h, w, generator=gen) - 0.5) * 32.0 + 0.5, torch.randn(n, 3, h * s, w * s, generator=gen)


def unshuffle_of(upscale):
    return {4: 1, 2: 2, 1: 4}[upscale]


def rdb_keys(nb):
    """The dense blocks in forward order: r -> "trunk.i.rdbj"."""
    return [f"trunk.{i}.rdb{j}" for i in range(nb) for j in (1, 2, 3)]


class Consts:
    """slope, res (the 0.2 of both residual scalings), fold_w[pos] (what multiplies conv5 in the mirrored passes of block pos = r % 3),
    fold_g[pos] (the scale of conv5's weight gradient), as float64 numbers."""

    def __init__(self, slope, res, fold_w, fold_g):
        self.slope, self.res, self.fold_w, self.fold_g = slope, res, fold_w, fold_g


_f = lambda v: float(np.float32(v))
DEVICE = Consts(_f(0.2), _f(0.2), [_f(0.2)] * 2 + [float(np.float32(0.2) * np.float32(0.2))], [_f(0.2)] * 2 + [_f(0.04)])
EXACT = Consts(0.2, 0.2, [0.2, 0.2, 0.2 * 0.2], [0.2, 0.2, 0.2 * 0.2])    # the model's own doubles: what float64 autograd differentiates


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def transposed(wt):
    """The weights of the backward-data pass of conv [cout,cin,3,3]: [cin,cout,3,3], taps flipped."""
    return wt.transpose(0, 1).flip(2, 3).contiguous()


def dgrad(g, wt, dtype, **epi):
    """g_in[n,c,y,x] = sum_{o,dy,dx} W[o,c,dy,dx] * g[n,o,y-dy+1,x-dx+1] (+ the epilogue): conv_ref.conv3x3 on the transposed, flipped
    weights."""
    return R.conv3x3(g, transposed(wt), dtype, **epi)[0]


def growth_slice(k):
    """The input channels of o_k (k = 1..4) inside the dense block's concatenation [x (64) | o_1 | o_2 | o_3 | o_4]; k = 0: x."""
    return slice(0, 64) if k == 0 else slice(64 + 32 * (k - 1), 64 + 32 * k)


def mirrored_weights(w, w5f, k):
    """The weight of the mirrored pass that yields g_o_k (k = 4..1) or g_x (k = 0), [cout, cin, 3, 3] over the concatenation
    [gin (64) | g_o_4 | g_o_3 | .. | g_o_{k+1}]: the slices W_j[:, growth_slice(k)]^T, flipped; w = [W_1 .. W_4], w5f = fold W_5."""
    sl = growth_slice(k)
    parts = [transposed(w5f[:, sl])] + [transposed(w[j - 1][:, sl]) for j in range(4, max(k, 0), -1)]
    return torch.cat(parts, dim=1)


def mirrored_inputs(gin, go, k):
    """[gin | g_o_4 | .. | g_o_{k+1}]; go: {j: g_o_j}."""
    return torch.cat([gin] + [go[j] for j in range(4, max(k, 0), -1)], dim=1)


def as_packed(w, fast, scale=None):
    """A weight as resr_pack_weights leaves it: w (times scale: one fp32 product), fast mode rounded once to f16."""
    w = w.detach().float().cpu()
    if scale is not None:
        w = w * torch.tensor(np.float32(scale), dtype=F32)
    return w.half().float() if fast else w


def packed_weights(sd, nb, fast):
    """{conv name: weight as packed} and, per dense block r, "<block>.conv5@fold": the conv5 of the mirrored passes, and
    "<block>.conv5@fold~": the OTHER legal evaluation of that f16 block minus it, per element.  resr_pack_weights is built
    with HIP's default -ffp-contract=fast, under which the fp32 product w * fold may be fused into the conversion: f16 of the exact product,
    one rounding instead of two (layout_ref.expected_f16_fused; tests/test_gpu_layout_kernels.py accepts either).  The two differ by one
    f16 ulp on the rare elements whose fp32 product rounds onto an f16 tie (about one in 2^13; measured on the MI355X: 2 of the 18432
    elements of one slice, and the device holds the fused value there).  fp32 blocks and unscaled f16 blocks have no such freedom."""
    out = {k[:-7]: as_packed(v, fast) for k, v in sd.items() if k.endswith(".weight")}
    for r, key in enumerate(rdb_keys(nb)):
        w = sd[key + ".conv5.weight"]
        out[key + ".conv5@fold"] = as_packed(w, fast, DEVICE.fold_w[r % 3])
        exact = w.detach().double().cpu().numpy() * DEVICE.fold_w[r % 3]          # (numpy converts float64 to f16 in one rounding)
        fused = torch.from_numpy(exact.astype(np.float16).astype(np.float32)) if fast else out[key + ".conv5@fold"]
        out[key + ".conv5@fold~"] = fused - out[key + ".conv5@fold"]
    return out


def exact_weights(sd, nb, consts=EXACT):
    out = {k[:-7]: v.detach().double().cpu() for k, v in sd.items() if k.endswith(".weight")}
    for r, key in enumerate(rdb_keys(nb)):
        out[key + ".conv5@fold"] = out[key + ".conv5"] * consts.fold_w[r % 3]
    return out


def _bias(sd, name):
    return sd[name + ".bias"].detach().float().cpu()


def to_nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a), 3, 1)))


def to_nhwc(t):
    return np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy())


def _kind(fast):
    return "f16" if fast else "f32"


def expected_slot(gy, fast):
    """The three words of the pre-scale slot after one backward pass on a zero-filled slot: (bits of max |g_y| 2^-6, 0, 0); strict: zeros."""
    if not fast:
        return [0, 0, 0]
    bits, b, flag = Y.absmax_slot(gy.detach().float().cpu().numpy(), PRESCALE_LOG2)
    return [int(bits), int(b), int(flag)]


def lift_of_slot(slot0):
    return float(Y.grad_prescale(int(slot0))) if slot0 else 1.0


def pool(g, positive, slope, dtype):
    """layout_ref.sumpool2x2 on an NCHW tensor of stored values: [n,c,2h,2w] -> [n,c,h,w] in `dtype` (numpy float64 / float32)."""
    pos = None if positive is None else to_nhwc(positive)
    return to_nchw(Y.sumpool2x2(to_nhwc(g.float()), pos, slope, dtype=dtype))


# ---- the per-pass rule ----------------------------------------------------------------------------------------------------------------
def judge_passes(dev, sd, x, gy, upscale, n_blocks, fast, backward=True):
    """One row per pass: {"pass", "kind", "ratio", "bad", "allowance", "worst", ...}; a pass is right when bad == 0.

    dev (CPU tensors, NCHW, in the storage type -- f16 fast, f32 strict -- unless noted; h, w: the trunk's, after the pixel-unshuffle):
      x_in [n,ci_pad,h,w]; ws: per dense block [n,192,h,w] = [x | o1 | o2 | o3 | o4]; sign: per dense block bool [n,128,h,w] (o1..o4);
      trunk_out, feat [n,64,h,w]; u1 [n,64,2h,2w]; u2, c3 [n,64,4h,4w]; sign_u2, sign_c3 bool; y fp32, ymask uint8 [n,3,4h,4w]
      backward: slot (three ints); g4 [n,32,4h,4w]; gA1 (conv4's backward-data result), gB, gA2 (upsampling2's), gM1, gA3 (upsampling1's,
      [n,64,2h,2w]), gF; gin: per dense block the gradient its mirrored passes READ ([n,64,h,w]; gin[3 nb - 1] = conv2's backward-data
      result); gS: per dense block {k: g_o_k [n,32,h,w]}; g_out: the g_x pass's result of block 0 before the add_inplace (the other
      blocks' results are the next gin); gsum: after it; g_xin [n,ci_pad,h,w]; grads {parameter name: fp32}; gx fp32.
      The backward rows need n_blocks == 1 (every pass observable); backward=False judges the forward alone.
    kind "bits": the result is defined bit for bit, bad = the number of elements whose bits differ (sign words: that differ from
    (stored > 0) where the stored value is not zero).  "zero": elements that must be exactly zero.  "mask": conv_ref.pass_mask_ok.  Else
    conv_ref.judge's kinds; A = conv_ref.allowance of the float32 evaluation on the same inputs."""
    rows = []
    nb, r_un = n_blocks, unshuffle_of(upscale)
    kind = _kind(fast)
    K = DEVICE
    ci_real = 3 * r_un * r_un
    W = packed_weights(sd, nb, fast)
    xf, gyf = x.detach().float().cpu(), gy.detach().float().cpu()

    def bits(name, got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        differ = Y.bits_differ(got.numpy(), want.numpy())
        worst = int(differ[0]) if differ.size else 0
        rows.append({"pass": name, "kind": "bits", "bad": int(differ.size), "ratio": float(differ.size > 0), "allowance": 0.0, "worst": worst,
                     "got": float(got.reshape(-1)[worst]), "want": float(want.reshape(-1)[worst])})

    def zero(name, got):
        nz = ~(got == 0)                                   # a NaN pattern left in a pad channel counts
        worst = int(nz.reshape(-1).to(torch.uint8).argmax()) if nz.numel() else 0
        rows.append({"pass": name, "kind": "zero", "bad": int(nz.sum()), "ratio": float(nz.any()), "allowance": 0.0, "worst": worst,
                     "got": float(got.reshape(-1)[worst]) if nz.numel() else 0.0, "want": 0.0})

    def signs(name, got, stored):
        differ = (got.bool() != (stored > 0)) & (stored != 0)
        worst = int(differ.reshape(-1).to(torch.uint8).argmax())
        rows.append({"pass": name, "kind": "bits", "bad": int(differ.sum()), "ratio": float(differ.any()), "allowance": 0.0, "worst": worst,
                     "got": float(got.reshape(-1)[worst]), "want": float(stored.reshape(-1)[worst] > 0),
                     "both_values": bool(got.any()) and not bool(got.all())})

    def num(name, got, r64, r32, k):
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        rec = R.judge(got, r64, r32, k)
        rows.append({"pass": name, "kind": k, "bad": rec["bad"], "ratio": rec["ratio"], "allowance": rec["allowance"], "worst": rec["worst"],
                     "got": rec["got"], "want": rec["want"], "kernel_err": rec["kernel_err"], "cpu32_err": rec["cpu32_err"]})
        return rec

    def num_w(name, got, r64, r32, k, extra):
        """num with a per-element term on top of the bound: what the freedom in a packed weight (packed_weights, "@fold~") can move."""
        A, e32 = R.allowance(r64, r32)
        b = R.bound(r64, A, k) + extra
        err = (got.double() - r64).abs()
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / b)
        worst = int(ratio.argmax())
        rows.append({"pass": name, "kind": k, "bad": int((~(err <= b)).sum()), "ratio": float(ratio.max()), "allowance": A, "worst": worst,
                     "got": float(got.reshape(-1)[worst]), "want": float(r64.reshape(-1)[worst]), "kernel_err": float(err.max()), "cpu32_err": e32,
                     "weight_term": float(extra.max())})

    def conv(name, got, inp, wname, k=None, **epi):
        b = _bias(sd, wname)
        return num(name, got, R.conv3x3(inp, W[wname], F64, bias=b, **epi)[0], R.conv3x3(inp, W[wname], F32, bias=b, **epi)[0], k or kind)

    def back(name, got, g, wt, **epi):
        num(name, got, dgrad(g, wt, F64, **epi), dgrad(g, wt, F32, **epi), kind)

    def wg(wname, xk, g, scale, up=False):
        dw64, db64 = R.wgrad(xk, g, scale, F64, up=up)
        dw32, db32 = R.wgrad(xk, g, scale, F32, up=up)
        num(f"dW {wname}", dev["grads"][wname + ".weight"], dw64, dw32, "f32")
        num(f"db {wname}", dev["grads"][wname + ".bias"], db64, db32, "f32")

    # ---- forward ----
    lay = Y.nchw_to_nhwc(xf.numpy(), r_un, dev["x_in"].shape[1], kind)["hi"]
    bits("x_in", dev["x_in"][:, :ci_real], to_nchw(lay)[:, :ci_real])
    zero("x_in pad", dev["x_in"][:, ci_real:])
    xin = dev["x_in"][:, :ci_real]
    conv("conv1", dev["ws"][0][:, :64], xin, "conv1")
    keys = rdb_keys(nb)
    for r, key in enumerate(keys):
        ws = dev["ws"][r]
        for k in range(1, 5):
            sl = growth_slice(k)
            conv(f"{key}.o{k}", ws[:, sl], ws[:, :sl.start], f"{key}.conv{k}", lrelu=True, slope=K.slope)
            signs(f"{key}.sign{k}", dev["sign"][r][:, 32 * (k - 1):32 * k], ws[:, sl])
        epi = dict(res0=ws[:, :64], s0=K.res, t0=1.0)
        if r % 3 == 2:
            epi.update(res1=dev["ws"][r - 2][:, :64], s1=K.res, t1=1.0)
        out = dev["ws"][r + 1][:, :64] if r + 1 < len(keys) else dev["trunk_out"]
        conv(f"{key}.conv5", out, ws, f"{key}.conv5", **epi)
    conv("conv2+skip", dev["feat"], dev["trunk_out"], "conv2", res0=dev["ws"][0][:, :64], s0=1.0, t0=1.0)
    conv("upsampling1", dev["u1"], dev["feat"], "upsampling1.0", up=True, lrelu=True, slope=K.slope)
    conv("upsampling2", dev["u2"], dev["u1"], "upsampling2.0", up=True, lrelu=True, slope=K.slope)
    signs("upsampling2 sign", dev["sign_u2"], dev["u2"])
    conv("conv3", dev["c3"], dev["u2"], "conv3.0", lrelu=True, slope=K.slope)
    signs("conv3 sign", dev["sign_c3"], dev["c3"])
    b4 = _bias(sd, "conv4")
    y64, pre64 = R.conv3x3(dev["c3"], W["conv4"], F64, bias=b4, clamp=True)
    rec = num("conv4 -> y", dev["y"], y64, R.conv3x3(dev["c3"], W["conv4"], F32, bias=b4, clamp=True)[0], "f32")
    wrong = R.pass_mask_ok(dev["ymask"], pre64, rec["allowance"])
    rows.append({"pass": "ymask", "kind": "mask", "bad": wrong, "ratio": float(wrong > 0), "allowance": rec["allowance"], "worst": 0,
                 "both_values": bool(dev["ymask"].bool().any()) and not bool(dev["ymask"].bool().all())})
    if not backward:
        return rows

    # ---- backward ----
    assert nb == 1, "the backward rows need every pass observable: n_blocks = 1"
    want = expected_slot(gyf, fast)
    slot = [int(v) for v in dev["slot"]]
    wrong = sum(a != b for a, b in zip(slot, want))
    rows.append({"pass": "slot", "kind": "bits", "bad": wrong, "ratio": float(wrong > 0), "allowance": 0.0, "worst": 0, "got": slot[0], "want": want[0]})
    lift = lift_of_slot(want[0])
    inv = 1.0 / lift
    ymask = dev["ymask"].numpy()
    g4 = to_nchw(Y.nchw_to_nhwc(gyf.numpy(), 1, 32, kind, mask=ymask, amax_bits=want[0] if fast else None)["hi"])
    bits("g4", dev["g4"][:, :3], g4[:, :3])
    zero("g4 pad", dev["g4"][:, 3:])
    g = dev["g4"][:, :3]
    wg("conv4", dev["c3"], g, inv)
    back("gA = conv4^T g4, masked", dev["gA1"], g, W["conv4"], mask=dev["sign_c3"].float(), slope=K.slope)
    wg("conv3.0", dev["u2"], dev["gA1"], inv)
    back("gB = conv3^T gA, masked", dev["gB"], dev["gA1"], W["conv3.0"], mask=dev["sign_u2"].float(), slope=K.slope)
    wg("upsampling2.0", dev["u1"], dev["gB"], inv, up=True)
    back("gA = upsampling2^T gB", dev["gA2"], dev["gB"], W["upsampling2.0"])
    pos = dev["u1"] > 0
    num("gM1 = pool gA, masked", dev["gM1"], pool(dev["gA2"], pos, K.slope, np.float64), pool(dev["gA2"], pos, K.slope, np.float32), kind)
    wg("upsampling1.0", dev["feat"], dev["gM1"], inv, up=True)
    back("gA = upsampling1^T gM1", dev["gA3"], dev["gM1"], W["upsampling1.0"])
    num("gF = pool gA", dev["gF"], pool(dev["gA3"], None, K.slope, np.float64), pool(dev["gA3"], None, K.slope, np.float32), kind)
    wg("conv2", dev["trunk_out"], dev["gF"], inv)
    back("gT = conv2^T gF", dev["gin"][len(keys) - 1], dev["gF"], W["conv2"])
    for r in range(len(keys) - 1, -1, -1):
        key, pos3 = keys[r], r % 3
        ws, gin, go = dev["ws"][r], dev["gin"][r], dev["gS"][r]
        w14 = [W[f"{key}.conv{k}"] for k in range(1, 5)]
        w5f = W[key + ".conv5@fold"]
        z14, w5d = [torch.zeros_like(v) for v in w14], W[key + ".conv5@fold~"].abs()
        free = lambda inp, k: R.correlate(inp.abs(), mirrored_weights(z14, w5d, k), F64)      # sum |g| |dW|: the mask and t0 only shrink it
        for k in range(4, 0, -1):
            wm, inp = mirrored_weights(w14, w5f, k), mirrored_inputs(gin, go, k)
            m = dev["sign"][r][:, 32 * (k - 1):32 * k].float()
            num_w(f"{key}.g_o{k}", go[k], R.conv3x3(inp, wm, F64, mask=m, slope=K.slope)[0], R.conv3x3(inp, wm, F32, mask=m, slope=K.slope)[0], kind,
                  free(inp, k))
        wm, inp = mirrored_weights(w14, w5f, 0), mirrored_inputs(gin, go, 0)
        epi = dict(res0=gin, s0=1.0, t0=K.res if pos3 == 2 else 1.0)
        if pos3 == 0:
            epi.update(res1=dev["gin"][r + 2], s1=1.0, t1=1.0)      # e: the gradient wrt the RRDB's output, which its third block read
        out = dev["gin"][r - 1] if r > 0 else dev["g_out"]
        num_w(f"{key}.g_x", out, R.conv3x3(inp, wm, F64, **epi)[0], R.conv3x3(inp, wm, F32, **epi)[0], kind, free(inp, 0))
        for k in range(1, 5):
            wg(f"{key}.conv{k}", ws[:, :growth_slice(k).start], go[k], inv)
        wg(f"{key}.conv5", ws, gin, K.fold_g[pos3] * inv)
    bits("add_inplace gF", dev["gsum"], torch.from_numpy(Y.add_plain(dev["g_out"].numpy(), dev["gF"].numpy())))
    wg("conv1", xin, dev["gsum"], inv)
    back("g_xin", dev["g_xin"][:, :ci_real], dev["gsum"], W["conv1"])
    zero("g_xin pad", dev["g_xin"][:, ci_real:])
    gx = Y.nhwc_to_nchw(to_nhwc(dev["g_xin"].float()), 3, r_un, amax_bits=want[0] if fast else None)
    bits("gx", dev["gx"], torch.from_numpy(np.ascontiguousarray(gx)))
    return rows


def bad_passes(rows):
    return {r["pass"]: r["bad"] for r in rows if r["bad"]}


# ---- the backward as one map of g_y, every store through `st` -------------------------------------------------------------------------
def _backward(fw, W, gy, nb, lift, st, K, fault=None):
    """fw: the forward's values and masks (x_in [n,ci_real,h,w], ws, sign, trunk_out, feat, u1, u2, c3, sign_u2, sign_c3, ymask -- float64 or
    stored); W: exact_weights / packed_weights; st: what a store does to a float64 result.  Returns every tensor judge_passes names, the
    gradient tensors in the lifted domain, grads and gx_lifted unlifted by the caller.  fault: FAULTS."""
    keys = rdb_keys(nb)
    d = lambda t: t.double()
    out = {"gS": [None] * len(keys), "gin": [None] * len(keys)}
    grads = {}
    inv = 1.0 / lift

    def wg(name, xk, g, scale=1.0, up=False):
        dw, db = R.wgrad(d(xk), d(g), 1.0, F64, up=up)
        grads[name + ".weight"], grads[name + ".bias"] = dw * (scale * inv), db * (scale * inv)

    def factor(positive):
        return torch.where(positive.bool(), torch.tensor(1.0, dtype=F64), torch.tensor(K.slope, dtype=F64))

    def conv(g, wt, mask=None, res0=None, t0=1.0, res1=None):
        """include/resr.h's order with this pass's constants as float64 numbers: mask, then v + t0 res0, then v + res1."""
        v = R.correlate(d(g), d(wt), F64)
        if mask is not None:
            v = v * factor(mask)
        if res0 is not None:
            v = v + t0 * d(res0)
        if res1 is not None:
            v = v + d(res1)
        return v

    def bwd(g, wt, **epi):
        return conv(g, transposed(wt), **epi)

    def epi_mask(m):
        return dict(mask=m)

    def sumpool(g, positive=None):
        acc = sum(d(g)[:, :, i::2, j::2] for i in range(2) for j in range(2))
        return acc if positive is None else acc * factor(positive)

    ymask = fw["ymask"].bool() if fault != "g4_ignores_ymask" else torch.ones_like(fw["ymask"]).bool()
    g4 = st(torch.where(ymask, gy.double() * lift, torch.zeros((), dtype=F64)))
    out["g4_real"] = g4
    wg("conv4", fw["c3"], g4)
    gA1 = st(bwd(g4, W["conv4"], **epi_mask(fw["sign_c3"])))
    if fault == "hr_dgrad_drops_last_column":
        gA1[..., -1] = 0
    out["gA1"] = gA1
    wg("conv3.0", fw["u2"], gA1)
    out["gB"] = gB = st(bwd(gA1, W["conv3.0"], **epi_mask(fw["sign_u2"])))
    if fault == "up2_wgrad_without_nearest":      # X[y, x] = u1[y, x] where u1 has such a pixel, nothing beyond: u1 read without the gather
        xq = torch.zeros_like(d(gB[:, :1]).expand(-1, 64, -1, -1)).contiguous()
        xq[:, :, :fw["u1"].shape[2], :fw["u1"].shape[3]] = d(fw["u1"])
        wg("upsampling2.0", xq, gB)
    else:
        wg("upsampling2.0", fw["u1"], gB, up=True)
    out["gA2"] = gA2 = st(bwd(gB, W["upsampling2.0"]))
    out["gM1"] = gM1 = st(sumpool(gA2, None if fault == "gM1_without_mask" else fw["u1"] > 0))
    wg("upsampling1.0", fw["feat"], gM1, up=True)
    out["gA3"] = gA3 = st(bwd(gM1, W["upsampling1.0"]))
    out["gF"] = gF = st(sumpool(gA3, (fw["feat"] > 0) if fault == "gF_with_mask" else None))
    wg("conv2", fw["trunk_out"], gF)
    gin = st(bwd(gF, W["conv2"]))
    e = None
    chain = [gin]                              # every gradient of the RDB chain so far, newest last: the ring's slots
    for r in range(len(keys) - 1, -1, -1):
        key, pos3 = keys[r], r % 3
        last_block = r == len(keys) - 1        # the faults sit in the first RRDB the backward visits
        out["gin"][r] = gin
        if pos3 == 2:
            e = gin
        w14 = [W[f"{key}.conv{k}"] for k in range(1, 5)]
        w5f = W[key + ".conv5@fold"]
        if fault == "rdb3_fold_0.2" and pos3 == 2 and last_block:
            w5f = W[key + ".conv5"].double() * K.fold_w[0]
        go = {}
        for k in range(4, 0, -1):
            if fault == "g_o4_conv5_slice_of_o3" and k == 4 and last_block:
                wm = transposed(d(w5f)[:, growth_slice(3)])
            else:
                wm = mirrored_weights([d(v) for v in w14], d(w5f), k)
            kk = 3 if (fault == "g_o4_mask_of_o3" and k == 4 and last_block) else k
            go[k] = st(conv(mirrored_inputs(d(gin), {j: d(v) for j, v in go.items()}, k), wm, **epi_mask(fw["sign"][r][:, 32 * (kk - 1):32 * kk])))
        out["gS"][r] = go
        t0 = K.res if pos3 == 2 else 1.0
        if fault == "rdb3_t0_1" and pos3 == 2 and last_block:
            t0 = 1.0
        epi = dict(res0=gin, t0=t0)
        if pos3 == 0:
            epi.update(res1=chain[-1] if (fault == "rdb1_skip_from_newest_slot" and r == len(keys) - 3) else e)
        gx_r = st(conv(mirrored_inputs(d(gin), {j: d(v) for j, v in go.items()}, 0), mirrored_weights([d(v) for v in w14], d(w5f), 0), **epi))
        for k in range(1, 5):
            wg(f"{key}.conv{k}", fw["ws"][r][:, :growth_slice(k).start], go[k])
        wg(f"{key}.conv5", fw["ws"][r], gin, K.fold_g[pos3])
        chain.append(gx_r)
        gin = gx_r
    out["g_out"] = gin
    out["grads"] = grads
    return out


# ---- the CPU stand-in for the device ---------------------------------------------------------------------------------------------------
# planted faults of emulate_passes; each is wrong in ONE pass (tests/test_generator_pass_ref.py, EXPECTED: the rows that must name it)
FAULTS = ("rdb3_fold_0.2", "rdb3_t0_1", "rdb1_skip_from_newest_slot", "g_o4_mask_of_o3", "g_o4_conv5_slice_of_o3", "gM1_without_mask",
          "gF_with_mask", "up2_wgrad_without_nearest", "g4_ignores_ymask", "g4_pad_nonzero", "hr_dgrad_drops_last_column",
          "db_conv1_without_unlift", "conv5_forward_residual_1.0")


def emulate_passes(sd, x, gy, upscale, n_blocks, fast=True, fault=None, fused_pack=False):
    """What one forward + backward (and the four stopped runs) leave, computed in float64 and rounded wherever the native pass stores
    (`dev` of judge_passes).  fused_pack: the folded conv5 blocks hold the other legal f16 evaluation (packed_weights).
    fault: None or one of FAULTS --
      rdb3_fold_0.2               the third block's mirrored passes run on 0.2 W_5 where 0.04 W_5 belongs (its g_o4..g_o1 and g_x)
      rdb3_t0_1                   the third block's g_x adds gin unscaled (t0 = 1 where 0.2 belongs)
      rdb1_skip_from_newest_slot  the first block's second residual is the ring's newest slot (its own gin) instead of e
      g_o4_mask_of_o3             the third block's g_o4 masked with o3's sign plane
      g_o4_conv5_slice_of_o3      the third block's g_o4 through conv5's input slice of o3
      gM1_without_mask            gM1 pooled without the LeakyReLU factor of u1
      gF_with_mask                gF pooled with a LeakyReLU factor (of feat)
      up2_wgrad_without_nearest   upsampling2's dW on a same-size X that is not the nearest-x2 of u1 (its columns one off)
      g4_ignores_ymask            g4 = layout(g_y * lift) without the pass mask
      g4_pad_nonzero              one pad channel of g4 holds a value in one pixel
      hr_dgrad_drops_last_column  conv4's backward-data pass leaves the last column of gA zero
      db_conv1_without_unlift     db of conv1 leaves without the 1 / lift
      conv5_forward_residual_1.0  the first block's conv5 epilogue scales the convolution by 1.0 instead of 0.2"""
    assert fault is None or fault in FAULTS, fault
    nb, r_un = n_blocks, unshuffle_of(upscale)
    tdt = F16 if fast else F32
    kind = _kind(fast)
    K = DEVICE
    st = lambda v: v.to(tdt)
    xf, gyf = x.detach().float().cpu(), gy.detach().float().cpu()
    ci_real = 3 * r_un * r_un
    ci_pad = (ci_real + 31) // 32 * 32
    W = packed_weights(sd, nb, fast)
    keys = rdb_keys(nb)
    if fused_pack:
        for key in keys:
            W[key + ".conv5@fold"] = W[key + ".conv5@fold"] + W[key + ".conv5@fold~"]

    def conv(inp, wname, **epi):
        return R.conv3x3(inp, W[wname], F64, bias=_bias(sd, wname), **epi)

    x_in = to_nchw(Y.nchw_to_nhwc(xf.numpy(), r_un, ci_pad, kind)["hi"])
    xin = x_in[:, :ci_real]
    n, _, h, w = x_in.shape
    ws = [torch.zeros(n, 192, h, w, dtype=tdt) for _ in keys]
    sign = []
    ws[0][:, :64] = st(conv(xin, "conv1")[0])
    trunk_out = None
    for r, key in enumerate(keys):
        for k in range(1, 5):
            sl = growth_slice(k)
            ws[r][:, sl] = st(conv(ws[r][:, :sl.start], f"{key}.conv{k}", lrelu=True, slope=K.slope)[0])
        sign.append(ws[r][:, 64:] > 0)
        epi = dict(res0=ws[r][:, :64], s0=1.0 if (fault == "conv5_forward_residual_1.0" and r == 0) else K.res, t0=1.0)
        if r % 3 == 2:
            epi.update(res1=ws[r - 2][:, :64], s1=K.res, t1=1.0)
        o = st(conv(ws[r], f"{key}.conv5", **epi)[0])
        if r + 1 < len(keys):
            ws[r + 1][:, :64] = o
        else:
            trunk_out = o
    feat = st(conv(trunk_out, "conv2", res0=ws[0][:, :64], s0=1.0, t0=1.0)[0])
    u1 = st(conv(feat, "upsampling1.0", up=True, lrelu=True, slope=K.slope)[0])
    u2 = st(conv(u1, "upsampling2.0", up=True, lrelu=True, slope=K.slope)[0])
    c3 = st(conv(u2, "conv3.0", lrelu=True, slope=K.slope)[0])
    y64, pre64 = conv(c3, "conv4", clamp=True)
    dev = {"x_in": x_in, "ws": ws, "sign": sign, "trunk_out": trunk_out, "feat": feat, "u1": u1, "u2": u2, "c3": c3, "sign_u2": u2 > 0,
           "sign_c3": c3 > 0, "y": y64.float(), "ymask": ((pre64 >= 0) & (pre64 <= 1)).to(torch.uint8)}
    dev["y_inference"] = dev["y"]
    slot = expected_slot(gyf, fast)
    lift = lift_of_slot(slot[0])
    fw = dict(dev, x_in=xin)
    b = _backward(fw, W, gyf, nb, lift, st, K, fault)
    g4 = torch.zeros(n, 32, 4 * h, 4 * w, dtype=tdt)
    g4[:, :3] = b["g4_real"]
    if fault == "g4_pad_nonzero":
        g4[0, 7, 2 * h, 2 * w] = 1.0
    gsum = torch.from_numpy(Y.add_plain(b["g_out"].numpy(), b["gF"].numpy()))
    dw, db = R.wgrad(xin, gsum, 1.0 / lift, F64)
    if fault == "db_conv1_without_unlift":
        db = db * lift
    grads = {k: v.float() for k, v in b["grads"].items()}
    grads["conv1.weight"], grads["conv1.bias"] = dw.float(), db.float()
    g_xin = torch.zeros(n, ci_pad, h, w, dtype=tdt)
    g_xin[:, :ci_real] = st(dgrad(gsum, W["conv1"], F64))
    gx = torch.from_numpy(np.ascontiguousarray(Y.nhwc_to_nchw(to_nhwc(g_xin.float()), 3, r_un, amax_bits=slot[0] if fast else None)))
    dev.update(slot=slot, lift=lift, g4=g4, gA1=b["gA1"], gB=b["gB"], gA2=b["gA2"], gM1=b["gM1"], gA3=b["gA3"], gF=b["gF"], gin=b["gin"],
               gS=b["gS"], g_out=b["g_out"], gsum=gsum, g_xin=g_xin, grads={k: grads[k] for k in sd}, gx=gx)
    return dev


def device_grads(dev):
    """{name: gradient} with "x"."""
    out = dict(dev["grads"])
    out["x"] = dev["gx"]
    return out


# ---- end to end, masks pinned ----------------------------------------------------------------------------------------------------------
def forward64(sd, x, upscale, n_blocks):
    """The float64 forward on the state dict's own (unrounded) values with the model's own doubles (0.2): the forward values and masks
    in the shape _backward takes, and "y"."""
    r_un = unshuffle_of(upscale)
    K = EXACT
    W = exact_weights(sd, n_blocks)
    keys = rdb_keys(n_blocks)
    lrelu = lambda v: torch.where(v > 0, v, v * K.slope)

    def conv(inp, name, up=False):
        return R.correlate(inp, W[name], F64, up) + sd[name + ".bias"].detach().double().view(1, -1, 1, 1)

    xin = torch.from_numpy(Y.pixel_unshuffle(x.detach().double().cpu().numpy(), r_un))
    ws, sign = [], []
    cur = conv(xin, "conv1")
    out1 = cur
    for r, key in enumerate(keys):
        feats = cur
        for k in range(1, 5):
            feats = torch.cat([feats, lrelu(conv(feats, f"{key}.conv{k}"))], dim=1)
        ws.append(feats)
        sign.append(feats[:, 64:] > 0)
        nxt = conv(feats, f"{key}.conv5") * K.res + cur
        if r % 3 == 2:
            nxt = nxt * K.res + ws[r - 2][:, :64]
        cur = nxt
    feat = out1 + conv(cur, "conv2")
    u1 = lrelu(conv(feat, "upsampling1.0", up=True))
    u2 = lrelu(conv(u1, "upsampling2.0", up=True))
    c3 = lrelu(conv(u2, "conv3.0"))
    pre = conv(c3, "conv4")
    return {"x_in": xin, "ws": ws, "sign": sign, "trunk_out": cur, "feat": feat, "u1": u1, "u2": u2, "c3": c3, "sign_u2": u2 > 0,
            "sign_c3": c3 > 0, "ymask": ((pre >= 0) & (pre <= 1)).to(torch.uint8), "y": pre.clamp(0.0, 1.0)}


def pinned_backward(W, fw, gy, upscale, n_blocks, names, round16=False, lift=None, consts=DEVICE):
    """{name: gradient} with "x": the whole backward in float64, the masks (sign planes, u1 > 0, ymask) and the forward values (the X of
    every weight gradient) taken from `fw` -- for fixed arguments one linear map of g_y.  W: the weights the map runs on (exact_weights, or
    packed_weights for what the device holds).  round16: every tensor the native pass stores (g4, gA in its three roles, gB, gM1, gF, the
    ring, the slabs, the add, g_xin) is rounded to f16 at `lift` (default: the native pass's own); sums stay exact."""
    r_un = unshuffle_of(upscale)
    g_y = gy.detach().double().cpu()
    if lift is None:
        lift = lift_of_slot(expected_slot(g_y, True)[0]) if round16 else 1.0
    st = (lambda v: v.half().double()) if round16 else (lambda v: v)
    b = _backward(fw, W, g_y, n_blocks, float(lift), st, consts)
    gsum = st(b["g_out"] + b["gF"])
    dw, db = R.wgrad(fw["x_in"].double(), gsum, 1.0 / lift, F64)
    grads = dict(b["grads"])
    grads["conv1.weight"], grads["conv1.bias"] = dw, db
    g_xin = st(dgrad(gsum, W["conv1"].double(), F64))
    grads["x"] = torch.from_numpy(np.ascontiguousarray(Y.pixel_shuffle(g_xin.numpy(), r_un))) / lift
    return {k: grads[k] for k in list(names) + ["x"]}


def rel_l2(got, ref):
    """Relative L2 per tensor, tests/test_gpu_generator.py's and tests/test_gpu_mx.py's measure."""
    return ((got.double().cpu() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300)).item()


def errors(grads, ref):
    return {k: rel_l2(grads[k], v) for k, v in ref.items()}


def worst_median(errs):
    v = sorted(errs.values())
    n = len(v)
    return v[-1], (v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2]))


def pinned_gate(grads, sd, dev, gy, upscale, n_blocks):
    """Section 3b, fast mode: `grads` ({name: gradient} with "x") against the float64 backward pinned on dev's stored activations, sign
    words and ymask and run on the weights fast mode packs (the linear map the device evaluates), next to the yardstick -- the same map
    with an f16 rounding at every store the native pass makes, at the same lift.  Returns the record; "ok" says worst and median are
    within 2 x the yardstick's, "condition" that the yardstick's own worst tensor is below YARDSTICK_WORST."""
    W = packed_weights(sd, n_blocks, True)
    r_un = unshuffle_of(upscale)
    fw = dict(dev, x_in=dev["x_in"][:, :3 * r_un * r_un])
    g64p = pinned_backward(W, fw, gy, upscale, n_blocks, sd, round16=False)
    e16p = pinned_backward(W, fw, gy, upscale, n_blocks, sd, round16=True)
    errs, yard = errors(grads, g64p), errors(e16p, g64p)
    worst, median = worst_median(errs)
    y_worst, y_median = worst_median(yard)
    return {"worst": worst, "median": median, "yardstick_worst": y_worst, "yardstick_median": y_median, "worst_tensor": max(errs, key=errs.get),
            "yardstick_worst_tensor": max(yard, key=yard.get), "condition": y_worst < YARDSTICK_WORST,
            "ok": worst <= 2.0 * y_worst and median <= 2.0 * y_median}
