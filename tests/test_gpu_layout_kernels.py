"""-m gpu: the kernels of csrc/layout.hip and csrc/pack.hip and the two scalar losses of csrc/loss.hip, each alone through the C ABI,
against the restatements of tests/layout_ref.py (validated on the CPU, mutations included, by tests/test_layout_ref.py).

How a result is judged (tests/layout_ref.py has the rule and the reasoning of every bound)
  * BIT FOR BIT: nchw_to_nhwc (hi, lo, q, padding channels), nhwc_to_nchw, absmax and its back-off, pack and pack_mx, EMA, the L1
    gradient, add_inplace in f32 and f16.  NaNs compare as NaNs; the q byte of a NaN is the byte rule on the stored f16 pattern.
  * against float64 with conv_ref's allowance: sumpool2x2 (kinds f32 / f16 / pair), the pair add (pair), the loss values (f32).
  * BCE: the allowance plus the stated error of exp through a one-ulp exp2; the ratio is recorded with and without that term.
  * every output lies between sentinel guards and is pre-filled with the sentinel: guards and the gaps between sub-tensors (hi | lo | q,
    packed blocks, slack) must survive, everything in range must have been written.
Every judgement goes to <diag_dir>/test_gpu_layout_kernels.json.

Measured on the MI355X (cases / bit-exact / worst ratio): nchw_to_nhwc 157 / 157, nhwc_to_nchw 39 / 39, absmax 53 / 53, pack 45 / 45,
pack_mx 9 / 9, EMA 31 / 31, L1 gradient 18 / 18, add_inplace 6 / 4 / 0.04 (the pair add), sumpool2x2 44 / - / 0.25 (f32), 0.99 (f16: the
store's own half ulp against a bound of 1.01 half ulps + A), 0.10 (pairs), L1 value 9 / - / 0.25, BCE gradient 18 / - / 0.250 (0.255
without the exp term), BCE value 18 / - / 0.248 (0.250).  A plain f16 packed block meets the compiler's fused evaluation of
f16(w * scale) (layout_ref.expected_f16_fused); the record of each chunk says which evaluation it matched.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import layout_ref as R
from tests.gpu_util import GUARD, SENT, Out, dev

pytestmark = pytest.mark.gpu
F32, F16, F64 = np.float32, np.float16, np.float64
SLOPE = float(F32(0.2))
RESR_ERR_ARG = -1
RECORDS = {}
S16, S32 = SENT[np.dtype(F16)], SENT[np.dtype(F32)]


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as pkg
    pkg._lib.lib()
    return pkg._lib


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    per = {}
    for rec in RECORDS.values():
        k = per.setdefault(rec["kernel"], {"cases": 0, "bit_exact": 0, "worst_ratio": 0.0})
        k["cases"] += 1
        k["bit_exact"] += bool(rec.get("exact"))
        k["worst_ratio"] = max(k["worst_ratio"], rec.get("ratio", 0.0))
        if "ratio_plain" in rec:
            k["worst_ratio_plain"] = max(k.get("worst_ratio_plain", 0.0), rec["ratio_plain"])
    with open(os.path.join(diag_dir, "test_gpu_layout_kernels.json"), "w") as f:
        json.dump({"kernels": per, "cases": RECORDS}, f, indent=1, sort_keys=True)


def ok(L, rc):
    assert rc == 0, (rc, L.lib().resr_last_error())


def refused(L, rc):
    assert rc == RESR_ERR_ARG, rc
    assert L.lib().resr_last_error()


def dt_of(L, kind):
    return {"f32": L.RESR_F32, "f16": L.RESR_F16, "f16x2": L.RESR_F16X2}[kind]


def np_of(kind):
    return F32 if kind == "f32" else F16


def exact(kernel, case, got, want, sentinel=None):
    bad = R.bits_differ(got, want, sentinel)
    RECORDS[f"{kernel}:{case}"] = {"kernel": kernel, "exact": bad.size == 0, "elements": int(np.asarray(want).size), "differ": int(bad.size)}
    if bad.size:
        g, w = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        raise AssertionError(f"{kernel}:{case}: {bad.size} of {w.size} elements differ, first at {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}")


def judged(kernel, case, rec):
    rec["kernel"] = kernel
    RECORDS[f"{kernel}:{case}"] = rec
    print(f"{kernel}:{case} cpu32_err {rec['cpu32_err']:.3e} allowance {rec['allowance']:.3e} kernel_err {rec['kernel_err']:.3e} ratio {rec['ratio']:.3f}"
          + (f" ratio_plain {rec['ratio_plain']:.3f}" if "ratio_plain" in rec else ""))
    assert rec["bad"] == 0, (kernel, case, rec)


def untouched(a, sent, what):
    i = np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])
    assert (i == sent).all(), f"{what}: {(i != sent).sum()} elements outside the tensors were written"


def slot_dev(bits, b=0, flag=0):
    return dev(np.array([bits, b, flag], dtype=np.uint32).view(np.int32))


# ---- nchw_to_nhwc ------------------------------------------------------------------------------------------------------------------
NCHW = R.nchw_cases()


@pytest.mark.parametrize("name", sorted(NCHW))
def test_nchw_to_nhwc(L, name):
    c = NCHW[name]
    kind, n, ch, h, w, r, cp = c["kind"], c["n"], c["c"], c["h"], c["w"], c["r"], c["c_pad"]
    src, mask = R.nchw_inputs(name, c)
    bits = R.AMAX_STATES.get(c["amax"])
    want = R.nchw_to_nhwc(src, r, cp, kind, mask, bits, c["q"])
    count = n * (h // r) * (w // r) * cp
    x2 = kind == "f16x2"
    lo_at = count + (24 if c["lo"] == "explicit" else 0) if x2 else 0
    q_at = lo_at + count + 40 if c["q"] else 0
    total = q_at + count if c["q"] else (lo_at + count if x2 else count)      # q: 64 bytes per pixel and chunk = the bytes of the hi tensor
    out = Out(total, np_of(kind))
    ds, dm = dev(src), (dev(mask) if mask is not None else None)
    slot = slot_dev(bits) if bits is not None else None
    mp = dm.data_ptr() if dm is not None else None
    if bits is None and not c["q"] and c["lo"] != "explicit":
        ok(L, L.lib().resr_nchw_to_nhwc(ds.data_ptr(), out.ptr, n, ch, h, w, r, cp, dt_of(L, kind), mp, None))
    else:
        lo_arg = (lo_at if c["lo"] == "explicit" else -1) if x2 else 0
        ok(L, L.lib().resr_debug_nchw_to_nhwc_q(ds.data_ptr(), out.ptr, n, ch, h, w, r, cp, dt_of(L, kind), mp, lo_arg,
                                                slot.data_ptr() if slot is not None else None, q_at, None))
    body = out.read(written=False)
    sent = S32 if kind == "f32" else S16
    hi = body[:count]
    exact("nchw_to_nhwc", name + ".hi", hi, want["hi"], sent)
    real = ch * r * r
    assert not hi.reshape(-1, cp)[:, real:].view(np.uint16 if kind != "f32" else np.uint32).any(), "padding channels of hi are not +0"
    if x2:
        lo = body[lo_at:lo_at + count]
        exact("nchw_to_nhwc", name + ".lo", lo, want["lo"], sent)
        assert not lo.reshape(-1, cp)[:, real:].view(np.uint16).any(), "padding channels of lo are not +0"
        untouched(body[count:lo_at], sent, "between hi and lo")
        if c["q"]:
            untouched(body[lo_at + count:q_at], sent, "between lo and q")
            q = body[q_at:q_at + count].view(np.uint8).reshape(want["q"].shape)
            # where the reference holds a NaN the stored pattern is the hardware's: the byte rule on what the kernel stored
            mix = lambda w_, g_: np.where(np.isnan(w_), g_.reshape(w_.shape), w_)
            exact("nchw_to_nhwc", name + ".q", q, R.q_records(mix(want["hi"], hi), mix(want["lo"], lo)))
            assert not q.reshape(-1, cp // 32, 2, 32).transpose(0, 2, 1, 3).reshape(-1, 2, cp)[:, :, real:].any(), "padding channels of q are not 0"


def test_nchw_to_nhwc_refusals(L):
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    lib = L.lib()
    refused(L, lib.resr_nchw_to_nhwc(p, p, 1, 3, 4, 4, 1, 12, L.RESR_F16, None, None))           # c_pad % 8
    refused(L, lib.resr_nchw_to_nhwc(p, p, 1, 3, 4, 4, 2, 8, L.RESR_F16, None, None))            # c r^2 > c_pad
    refused(L, lib.resr_nchw_to_nhwc(p, p, 1, 3, 3, 4, 2, 32, L.RESR_F16, None, None))           # h % r
    refused(L, lib.resr_debug_nchw_to_nhwc_q(p, p, 1, 3, 4, 4, 1, 32, L.RESR_F16, None, 0, None, 512, None))     # q without pairs
    refused(L, lib.resr_debug_nchw_to_nhwc_q(p, p, 1, 3, 4, 4, 1, 8, L.RESR_F16X2, None, -1, None, 512, None))   # q with c_pad % 32
    torch.cuda.synchronize()
    assert not buf.any()


# ---- nhwc_to_nchw ------------------------------------------------------------------------------------------------------------------
NHWC = R.nhwc_cases()


@pytest.mark.parametrize("name", sorted(NHWC))
def test_nhwc_to_nchw(L, name):
    c = NHWC[name]
    kind, n, ch, h, w, r, stride = c["kind"], c["n"], c["c"], c["h"], c["w"], c["r"], c["stride"]
    v32, hi, lo = R.nhwc_loaded(name, c)
    bits = R.AMAX_STATES.get(c["amax"])
    want = R.nhwc_to_nchw(v32, ch, r, bits)
    gap = np.full(16 if c["lo"] == "explicit" else 0, np.nan, dtype=F16)
    flat = hi.reshape(-1) if lo is None else np.concatenate([hi.reshape(-1), gap, lo.reshape(-1)])
    src = dev(flat)
    out = Out(n * ch * h * w, F32)
    slot = slot_dev(bits) if bits is not None else None
    if bits is None and c["lo"] != "explicit":
        ok(L, L.lib().resr_nhwc_to_nchw(src.data_ptr(), out.ptr, n, ch, h, w, r, stride, dt_of(L, kind), None))
    else:
        lo_arg = 0 if lo is None else (hi.size + gap.size if c["lo"] == "explicit" else -1)
        ok(L, L.lib().resr_debug_nhwc_to_nchw(src.data_ptr(), out.ptr, n, ch, h, w, r, stride, dt_of(L, kind), lo_arg,
                                              slot.data_ptr() if slot is not None else None, None))
    exact("nhwc_to_nchw", name, out.read(), want, S32)


# ---- absmax ------------------------------------------------------------------------------------------------------------------------
ABSMAX = R.absmax_cases()


@pytest.mark.parametrize("name", sorted(ABSMAX))
def test_absmax(L, name):
    c = ABSMAX[name]
    x = R.absmax_input(c)
    want = R.absmax_slot(x, c["t"], c["slot1"], c["slot2"])
    buf = torch.zeros(c["count"] + 8, device="cuda")
    buf[c["offset"]:c["offset"] + c["count"]] = dev(x)
    slot = Out(3, F32).load(np.array([0x12345678, c["slot1"], c["slot2"]], dtype=np.uint32).view(F32))   # slot[0]: stale bits the pass must overwrite
    ok(L, L.lib().resr_debug_absmax(buf.data_ptr() + 4 * c["offset"], c["count"], slot.ptr, c["t"], None))
    got = slot.read(written=False).view(np.uint32)
    m = int(got[0])
    if want[0] == "nan":
        good = (m & 0x7F800000) == 0x7F800000 and (m & 0x007FFFFF) != 0 and not m >> 31
    else:
        good = m == want[0]
    RECORDS[f"absmax:{name}"] = {"kernel": "absmax", "exact": bool(good) and (int(got[1]), int(got[2])) == want[1:], "got": [int(v) for v in got],
                                 "want": [str(v) for v in want]}
    assert good and (int(got[1]), int(got[2])) == want[1:], (name, [hex(int(v)) for v in got], want)
    if want[0] != "nan":                                              # what the layout passes make of the slot
        assert R.grad_prescale(m) * R.grad_prescale(m, inverse=True) == 1.0


def test_absmax_refusals(L):
    buf = torch.ones(16, device="cuda")
    slot = Out(3, F32)
    for count, t in ((4, 65), (4, -65), (0, 0), (-4, 0)):
        refused(L, L.lib().resr_debug_absmax(buf.data_ptr(), count, slot.ptr, t, None))
    refused(L, L.lib().resr_debug_absmax(None, 4, slot.ptr, 0, None))
    refused(L, L.lib().resr_debug_absmax(buf.data_ptr(), 4, None, 0, None))
    untouched(slot.read(written=False), S32, "the slot of a refused call")


# ---- sumpool2x2 --------------------------------------------------------------------------------------------------------------------
SUMPOOL = R.sumpool_cases()


@pytest.mark.parametrize("name", sorted(SUMPOOL))
def test_sumpool2x2(L, name):
    c = SUMPOOL[name]
    kind, n, ho, wo, ch = c["kind"], c["n"], c["ho"], c["wo"], c["c"]
    xh, xl, mh, ml, pos = R.sumpool_operands(name, c)
    count, x2, dt = n * ho * wo * ch, kind == "f16x2", np_of(kind)
    if not c["plane"]:
        src = dev(xh.reshape(-1) if not x2 else np.concatenate([xh.reshape(-1), xl.reshape(-1)]))
        mask = dev(mh.reshape(-1) if not x2 else np.concatenate([mh.reshape(-1), ml.reshape(-1)])) if c["mask"] else None
        out = Out(count * (2 if x2 else 1), dt)
        ok(L, L.lib().resr_sumpool2x2(src.data_ptr(), out.ptr, mask.data_ptr() if mask is not None else None, n, ho, wo, ch, dt_of(L, kind),
                                      SLOPE, None))
        body = out.read()
        ghi, glo = body[:count], (body[count:] if x2 else None)
    else:
        # the generator's form: plane 1 of chunk-planar pair tensors [hi plane 0 | hi plane 1 | lo plane 0 | lo plane 1]
        junk_in, junk_out = np.full(4 * count, np.nan, dtype=F16), np.full(count, np.nan, dtype=F16)
        src = dev(np.concatenate([junk_in, xh.reshape(-1), junk_in, xl.reshape(-1)]))
        mask = dev(np.concatenate([junk_out, mh.reshape(-1), junk_out, ml.reshape(-1)])) if c["mask"] else None
        out = Out(4 * count, F16)
        ok(L, L.lib().resr_debug_sumpool2x2(src.data_ptr() + 2 * 4 * count, out.ptr + 2 * count, mask.data_ptr() + 2 * count if mask is not None else None,
                                            n, ho, wo, ch, L.RESR_F16X2, SLOPE, 2 * 4 * count, 2 * count, None))
        body = out.read(written=False)
        untouched(body[:count], S16, "hi plane 0")
        untouched(body[2 * count:3 * count], S16, "lo plane 0")
        ghi, glo = body[count:2 * count], body[3 * count:]
        assert not (ghi.view(np.uint16) == S16).any() and not (glo.view(np.uint16) == S16).any(), "elements in range never written"
    got = ghi.astype(F64) if not x2 else R.pair_value(ghi, glo)
    judged("sumpool2x2", name, R.judge_sumpool(c, got, xh, xl, pos))
    if c["mask"] and x2:                                              # the planted sign-rule corners one by one: the other branch is >= 0.8 away
        exact_v = R.sumpool2x2(R.pair_value(xh, xl), pos)
        idx = R.planted_pair_mask(np.random.default_rng(0), pos.shape)[2]
        assert np.abs(got.reshape(-1)[idx] - exact_v.reshape(-1)[idx]).max() <= 1e-4


def test_sumpool_refusals(L):
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    for dtype, ch in ((L.RESR_F32, 6), (L.RESR_F16, 12), (L.RESR_F16X2, 4), (L.RESR_F32, 0)):
        refused(L, L.lib().resr_sumpool2x2(p, p, None, 1, 1, 1, ch, dtype, SLOPE, None))
        refused(L, L.lib().resr_debug_sumpool2x2(p, p, None, 1, 1, 1, ch, dtype, SLOPE, -1, -1, None))
    refused(L, L.lib().resr_sumpool2x2(p, p, None, 0, 1, 1, 8, L.RESR_F16, SLOPE, None))
    torch.cuda.synchronize()
    assert not buf.any()


# ---- add_inplace -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.ADD_COUNTS_E)
@pytest.mark.parametrize("kind", R.DTYPES)
def test_add_inplace(L, kind, k):
    e = 4 if kind == "f32" else 8
    count = k * e
    rng = np.random.default_rng(count)
    a32, b32 = R.planted(rng, count)[:count], (rng.standard_normal(count) * 3).astype(F32)
    a32[~np.isfinite(a32)] = 2.5
    a32 = np.clip(a32, -30000, 30000)
    if kind != "f16x2":
        a, b = a32.astype(np_of(kind)), b32.astype(np_of(kind))
        out = Out(count, np_of(kind)).load(a)
        src = dev(b)
        ok(L, L.lib().resr_debug_add_inplace(out.ptr, src.data_ptr(), count, dt_of(L, kind), 0, 0, None))
        exact("add_inplace", f"{kind}-{count}", out.read(), R.add_plain(a, b), S32 if kind == "f32" else S16)
        return
    (ah, al), (bh, bl) = R.pair_split(a32), R.pair_split(b32)
    dst_lo, src_lo = count + 8, count + 24
    out = Out(dst_lo + count, F16)
    out.t[GUARD:GUARD + count] = dev(ah)
    out.t[GUARD + dst_lo:GUARD + dst_lo + count] = dev(al)
    src = dev(np.concatenate([bh, np.full(24, np.nan, dtype=F16), bl]))
    ok(L, L.lib().resr_debug_add_inplace(out.ptr, src.data_ptr(), count, L.RESR_F16X2, dst_lo, src_lo, None))
    body = out.read(written=False)
    untouched(body[count:dst_lo], S16, "between dst's hi and lo")
    got = R.pair_value(body[:count], body[dst_lo:])
    judged("add_inplace", f"f16x2-{count}", R.judge(got, R.pair_value(ah, al) + R.pair_value(bh, bl), R.add_pair32(ah, al, bh, bl), "pair"))


def test_add_inplace_refusals(L):
    buf = torch.zeros(1024, device="cuda")
    p = buf.data_ptr()
    lib = L.lib()
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 6, L.RESR_F32, 0, 0, None))
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 12, L.RESR_F16, 0, 0, None))
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 12, L.RESR_F16X2, 64, 64, None))
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 0, L.RESR_F32, 0, 0, None))
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 8, L.RESR_F16X2, 0, 0, None))           # pairs without their lo offsets
    refused(L, lib.resr_debug_add_inplace(p, p + 2048, 8, L.RESR_F16X2, 64, -1, None))
    torch.cuda.synchronize()
    assert not buf.any()


# ---- pack / pack_mx ----------------------------------------------------------------------------------------------------------------
def upload_table(L, chunks, scale_dev):
    host = (L.PackChunk * len(chunks))()
    for i, ch in enumerate(chunks):
        host[i] = L.PackChunk(ch.src_off, ch.dst_off, ch.src_cout, ch.src_cin, ch.m_off, ch.m_count, ch.k_off, ch.k_count, ch.mt, ch.transposed,
                              ch.scale, ch.virtual4x4, scale_dev.data_ptr() if ch.scale_value is not None else None)
    return L.upload_chunks(host, "cuda")


@pytest.mark.parametrize("kind", R.DTYPES)
def test_pack_weights_every_element(L, kind):
    arena, chunks, elems, sv = R.pack_table()
    nb, es = (3, 2) if kind == "f16x2" else (1, 4 if kind == "f32" else 2)
    scale_dev = dev(np.array([sv], dtype=F32))
    table, ad = upload_table(L, chunks, scale_dev), dev(arena)
    out = Out(elems * nb * es + 16384, np.uint8)
    ok(L, L.lib().resr_pack_weights(table.data_ptr(), len(chunks), ad.data_ptr(), out.ptr, dt_of(L, kind), None))
    body = out.read(written=False)
    seen = np.zeros(body.size, dtype=bool)
    for i, ch in enumerate(chunks):
        want = R.expected_blocks(arena, ch, kind)
        total = R.block_elems(ch.mt)
        for j, wb in enumerate(want):
            lo = (ch.dst_off * nb + j * total) * es
            assert not seen[lo:lo + total * es].any()
            seen[lo:lo + total * es] = True
            got = R.unpack_block(body[lo:lo + total * es].view(np_of(kind)), ch.mt)
            if kind != "f16":
                exact("pack_kernel", f"{kind}-chunk{i}-W{j}", got, wb)
                continue
            bad, apart = R.f16_block_differs(got, arena, ch)            # either legal evaluation of f16(w * scale): layout_ref.expected_f16_fused
            RECORDS[f"pack_kernel:f16-chunk{i}"] = {"kernel": "pack_kernel", "exact": bad.size == 0, "elements": int(wb.size), "differ": int(bad.size),
                                                   "evaluations_apart": apart, "unfused": int(R.bits_differ(got, wb).size == 0)}
            assert bad.size == 0, f"pack_kernel:f16-chunk{i}: {bad.size} elements are neither rounding of w * scale, first at {bad[0]}"
    untouched(body[~seen], SENT[np.dtype(np.uint8)], "between the blocks and in the slack")
    assert (~seen).sum() == 16384 + 512 * nb * es


def test_pack_weights_mx_every_byte(L):
    arena, chunks, elems, sv = R.pack_table()
    scale_dev = dev(np.array([sv], dtype=F32))
    table, ad = upload_table(L, chunks, scale_dev), dev(arena)
    out = Out(elems * 2 + 16384, np.uint8)
    ok(L, L.lib().resr_pack_weights_mx(table.data_ptr(), len(chunks), ad.data_ptr(), out.ptr, None))
    body = out.read(written=False)
    seen = np.zeros(body.size, dtype=bool)
    for i, ch in enumerate(chunks):
        lo, nbytes = 2 * ch.dst_off, 9 * ch.mt * 2048
        seen[lo:lo + nbytes] = True
        exact("pack_mx_kernel", f"chunk{i}", R.unpack_mx_block(body[lo:lo + nbytes], ch.mt), R.expected_mx(arena, ch))
    untouched(body[~seen], SENT[np.dtype(np.uint8)], "between the MX blocks and in the slack")
    assert (~seen).sum() == 16384 + 1024


def test_pack_refusals(L):
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    refused(L, L.lib().resr_pack_weights(p, 0, p, p, L.RESR_F16, None))
    refused(L, L.lib().resr_pack_weights(None, 1, p, p, L.RESR_F16, None))
    refused(L, L.lib().resr_pack_weights_mx(p, 0, p, p, None))


# ---- EMA ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", R.EMA_COUNTS)
def test_ema_three_updates(L, count):
    rng = np.random.default_rng(count)
    big = count > 1 << 20
    for decay in (R.EMA_DECAYS[:1] if big else R.EMA_DECAYS):
        for shift in ((0,) if big else (0, 1)):                        # shift 1: both pointers 4 bytes past a 16-byte boundary (scalar kernel)
            s0 = rng.standard_normal(count + shift).astype(F32)
            shadow = Out(count + shift, F32).load(s0)
            want = s0[shift:].copy()
            for step in range(3):
                p = rng.standard_normal(count + shift).astype(F32)
                pd = dev(p)
                ok(L, L.lib().resr_ema_update(shadow.ptr + 4 * shift, pd.data_ptr() + 4 * shift, count, decay, None))
                want = R.ema(want, p[shift:], decay)
            got = shadow.read()
            exact("ema_scalar_kernel" if shift else "ema_kernel", f"n{count}-decay{decay}", got[shift:], want, S32)
            if shift:
                assert got[0] == s0[0], "the element in front of the shadow was written"


def test_ema_refusals(L):
    buf = torch.zeros(64, device="cuda")
    refused(L, L.lib().resr_ema_update(buf.data_ptr(), buf.data_ptr() + 128, 0, 0.999, None))
    refused(L, L.lib().resr_ema_update(None, buf.data_ptr(), 4, 0.999, None))


# ---- L1 mean / BCE with a constant label -------------------------------------------------------------------------------------------
WEIGHT = 0.37


def run_loss(L, fn, scratch, count, with_grad=True):
    loss, grad = Out(1, F32), (Out(count, F32) if with_grad else None)
    ok(L, fn(loss.ptr, grad.ptr if grad is not None else None, scratch.data_ptr()))
    value = loss.read()
    return value, (grad.read() if grad is not None else None)


@pytest.mark.parametrize("count", R.LOSS_COUNTS)
def test_l1_mean(L, count):
    a, b, _ = R.loss_inputs(count)
    da, db = dev(a), dev(b)
    scratch = torch.zeros(L.lib().resr_loss_scratch_bytes() // 4, dtype=torch.int32, device="cuda")
    fn = lambda loss, grad, sc: L.lib().resr_l1_mean(da.data_ptr(), db.data_ptr(), count, WEIGHT, loss, grad, sc, None)
    l1, g1 = run_loss(L, fn, scratch, count)
    l2, g2 = run_loss(L, fn, scratch, count)
    l3, _ = run_loss(L, fn, scratch, count, with_grad=False)
    assert l1.view(np.uint32)[0] == l2.view(np.uint32)[0] == l3.view(np.uint32)[0], "two calls on one scratch (and grad = NULL) differ"
    assert int(scratch[0].item()) == 0, "the arrival counter was not re-armed"
    l64, _ = R.l1_mean(a, b, WEIGHT)
    l32, g32 = R.l1_mean(a, b, WEIGHT, F32)
    exact("l1_mean.grad", f"n{count}", g1, g32, S32)
    exact("l1_mean.grad", f"n{count}-again", g2, g32, S32)
    judged("l1_mean.loss", f"n{count}", R.judge(l1, l64, l32, "f32"))


@pytest.mark.parametrize("label", [0.0, 1.0])
@pytest.mark.parametrize("count", R.LOSS_COUNTS)
def test_bce_logits_const(L, count, label):
    _, _, x = R.loss_inputs(count)
    dx = dev(x)
    scratch = torch.zeros(L.lib().resr_loss_scratch_bytes() // 4, dtype=torch.int32, device="cuda")
    fn = lambda loss, grad, sc: L.lib().resr_bce_logits_const(dx.data_ptr(), count, label, WEIGHT, loss, grad, sc, None)
    l1, g1 = run_loss(L, fn, scratch, count)
    l2, g2 = run_loss(L, fn, scratch, count)
    l3, _ = run_loss(L, fn, scratch, count, with_grad=False)
    assert l1.view(np.uint32)[0] == l2.view(np.uint32)[0] == l3.view(np.uint32)[0], "two calls on one scratch (and grad = NULL) differ"
    assert R.bits_differ(g1, g2).size == 0
    assert int(scratch[0].item()) == 0, "the arrival counter was not re-armed"
    l64, g64 = R.bce_const(x, label, WEIGHT)
    l32, g32 = R.bce_const(x, label, WEIGHT, F32)
    ge, le = R.bce_exp_terms(x, WEIGHT)
    judged("bce_logits_const.grad", f"n{count}-label{label}", R.judge(g1, g64, g32, "f32", ge))
    judged("bce_logits_const.loss", f"n{count}-label{label}", R.judge(l1, l64, l32, "f32", le))


def test_loss_refusals(L):
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    lib = L.lib()
    scratch = p + 8192
    refused(L, lib.resr_l1_mean(p + 4, p + 1024, 8, 1.0, p + 2048, p + 3072, scratch, None))     # a misaligned operand
    refused(L, lib.resr_l1_mean(p, p + 1028, 8, 1.0, p + 2048, p + 3072, scratch, None))
    refused(L, lib.resr_l1_mean(p, p + 1024, 8, 1.0, p + 2048, p + 3076, scratch, None))
    refused(L, lib.resr_bce_logits_const(p + 4, 8, 1.0, 1.0, p + 2048, p + 3072, scratch, None))
    refused(L, lib.resr_bce_logits_const(p, 8, 1.0, 1.0, p + 2048, p + 3076, scratch, None))
    refused(L, lib.resr_l1_mean(p, p + 1024, 0, 1.0, p + 2048, None, scratch, None))
    refused(L, lib.resr_bce_logits_const(p, 0, 1.0, 1.0, p + 2048, None, scratch, None))
    refused(L, lib.resr_l1_mean(p, p + 1024, 8, 1.0, p + 2048, None, None, None))
    torch.cuda.synchronize()
    assert not buf.any()
