"""CPU: tests/layout_ref.py is right (against torch's own operators, float64 autograd and torch.float8_e5m2), and its rule has, at the
very cases tests/test_gpu_layout_kernels.py runs, the power that module relies on: the reference passes its own rule, every wrong
kernel below is rejected.  A "wrong kernel" is the reference with ONE defect, stored as a correct kernel would store it."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_helpers_ref as D
from tests import layout_ref as R

F32, F16, F64 = np.float32, np.float16, np.float64
ALL_F16 = np.arange(65536, dtype=np.uint16).view(F16)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the references are right ------------------------------------------------------------------------------------------------------
def test_bf8_byte_rule_against_torch_on_every_f16_pattern():
    got = R.bf8_bits(ALL_F16)
    want = tt(ALL_F16).to(torch.float8_e5m2).view(torch.uint8).numpy()
    nan = np.isnan(ALL_F16)
    assert np.array_equal(got[~nan], want[~nan])
    wf = tt(want).view(torch.float8_e5m2).float().numpy()
    assert np.isnan(wf[nan]).all()
    # The byte rule rounds a NaN's payload like any significand: the NaN every fp32 -> f16 conversion of the hardware and of numpy makes
    # (0x7e00, either sign) stays one, as does every payload 0x081 .. 0x37f; up to 0x080 the byte is an infinity, above it the carry
    # leaves a zero of the other sign.  The GPU test therefore states the q byte of a NaN from the stored f16 pattern, not as "a NaN".
    p = ALL_F16.view(np.uint16) & 0x7FFF
    keeps = (p > 0x7C80) & (p < 0x7F80)
    assert ((got[keeps] & 0x7F) > 0x7C).all() and keeps[0x7E00] and keeps[0xFE00]
    assert ((got[nan & (p <= 0x7C80)] & 0x7F) == 0x7C).all() and ((got[p >= 0x7F80] & 0x7F) == 0).all()


def test_f16_rounding_and_pair_split():
    v = R.SPECIALS
    assert np.array_equal(R.f16_rne(v).view(np.uint16)[~np.isnan(v)], tt(v).half().numpy().view(np.uint16)[~np.isnan(v)])
    one = R.f16_rne(F32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.996, 65520.0, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -26]))
    assert one.tolist()[:3] == [1.0, 1.0 + 2.0 ** -9, 65504.0] and np.isinf(one[3])
    assert one.astype(F64).tolist()[4:] == [2.0 ** -23, 2.0 ** -23, 0.0]          # subnormal ties go to the even neighbour; below 2^-25: zero
    hi, lo = R.pair_split(F32([2.0 ** -26, -1.3 * 2.0 ** -27, 0.1]))
    assert hi.tolist()[:2] == [0.0, -0.0] and lo[0] == F16(2.0 ** -14) and lo[1] < 0    # hi is zero, lo carries the value
    assert abs(R.pair_value(hi, lo)[2] - float(F32(0.1))) <= D.pair_bound(0.1)
    x = np.random.default_rng(0).standard_normal(4096).astype(F32)
    hi, lo = R.pair_split(x)
    assert (np.abs(R.pair_value(hi, lo) - x.astype(F64)) <= D.pair_bound(x)).all()
    assert np.array_equal(R.pair_load32(hi, lo), (hi.astype(F64) + lo.astype(F64) / 4096).astype(F32))


@pytest.mark.parametrize("r", [1, 2, 4])
def test_pixel_shuffles_against_torch(r):
    x = np.random.default_rng(r).standard_normal((2, 3, 8, 12)).astype(F32)
    u = R.pixel_unshuffle(x, r)
    assert np.array_equal(u, F.pixel_unshuffle(tt(x), r).numpy())
    assert np.array_equal(R.pixel_shuffle(u, r), x) and np.array_equal(R.pixel_shuffle(u, r), F.pixel_shuffle(tt(u), r).numpy())
    out = R.nchw_to_nhwc(x, r, 64, "f16")["hi"]
    assert out.shape == (2, 8 // r, 12 // r, 64) and not out[..., 3 * r * r:].any()
    assert np.array_equal(out[..., :3 * r * r], F.pixel_unshuffle(tt(x), r).permute(0, 2, 3, 1).half().numpy())
    back = R.nhwc_to_nchw(out.astype(F32), 3, r)
    assert np.array_equal(back, tt(x).half().float().numpy())


def test_grad_prescale_is_the_documented_power_of_two():
    for m, s in ((1.5 * 2.0 ** -20, 2.0 ** 20), (2.0 ** -20, 2.0 ** 20), (0.999, 2.0), (0.5, 2.0), (2.0 ** -126, 2.0 ** 126), (1.0, 1.0), (3.0, 1.0),
                 (0.0, 1.0), (2.0 ** -127, 1.0), (math.inf, 1.0), (math.nan, 1.0)):
        bits = R.float_to_bits(m)
        assert R.grad_prescale(bits) == F32(s), m
        assert float(R.grad_prescale(bits)) * float(R.grad_prescale(bits, inverse=True)) == 1.0
        if s != 1.0:
            assert 1.0 <= m * s < 2.0
    assert R.grad_prescale(None) == 1.0


def test_absmax_slot_states():
    v = F32([0.25, -3.0, 1.0])
    assert R.absmax_slot(v, 0) == (R.float_to_bits(3.0), 0, 0)
    assert R.absmax_slot(v, 6) == (R.float_to_bits(3.0 / 64), 0, 0)
    assert R.absmax_slot(v, 6, 0, 1) == (R.float_to_bits(3.0 / 64 * 16), 4, 0)        # the step of 4
    assert R.absmax_slot(v, 6, 38, 1) == (R.float_to_bits(3.0 / 64 * 2.0 ** 40), 40, 0)    # the cap
    assert R.absmax_slot(v, 6, 100, 0)[1] == 40
    assert R.absmax_slot(F32([1.5 * 2.0 ** 100]), 0, 40) == (R.float_to_bits(1.5 * 2.0 ** 127), 40, 0)     # exponent held at 254
    assert R.absmax_slot(F32([0.0, -0.0]), 0, 8, 1) == (0, 12, 0)
    assert R.absmax_slot(F32([2.0 ** -130]), 0, 8) == (R.float_to_bits(2.0 ** -130), 8, 0)               # subnormal: left alone
    assert R.absmax_slot(F32([1.0, -np.inf]), 6, 8) == (0x7F800000, 8, 0)
    assert R.absmax_slot(F32([np.inf, np.nan]), 6, 8)[0] == "nan"
    assert R.absmax_slot(F32([2.0 ** -70]), 64, 8) == (R.float_to_bits(2.0 ** -134), 8, 0)


def test_sumpool_against_avg_pool():
    x = np.random.default_rng(1).standard_normal((2, 6, 10, 8))
    want = 4 * F.avg_pool2d(tt(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    assert np.abs(R.sumpool2x2(x) - want).max() < 1e-14
    assert np.abs(R.sumpool2x2(x.astype(F32), dtype=F32).astype(F64) - want).max() < 1e-5
    pos = x[:, ::2, ::2] > 0
    assert np.abs(R.sumpool2x2(x, pos, 0.2) - want * np.where(pos, 1.0, float(F32(0.2)))).max() < 1e-14


@pytest.mark.parametrize("count", [1, 5, 1025])
def test_losses_against_torch_float64(count):
    a, b, x = R.loss_inputs(count)
    w = 0.37
    w32 = float(F32(w))
    ta = tt(a).double().requires_grad_(True)
    l = F.l1_loss(ta, tt(b).double()) * w32
    l.backward()
    loss, grad = R.l1_mean(a, b, w)
    assert abs(loss - l.item()) < 1e-14 and np.abs(grad - ta.grad.numpy()).max() < 1e-16
    l32, g32 = R.l1_mean(a, b, w, F32)
    assert abs(float(l32) - l.item()) < 1e-5 and np.abs(g32 - ta.grad.numpy()).max() < 1e-7 * w32 / count + 1e-12
    for label in (0.0, 1.0):
        tx = tt(x).double().requires_grad_(True)
        l = F.binary_cross_entropy_with_logits(tx, torch.full_like(tx, label)) * w32
        l.backward()
        loss, grad = R.bce_const(x, label, w)
        assert abs(loss - l.item()) < 1e-13 * max(1.0, abs(l.item())) and np.abs(grad - tx.grad.numpy()).max() < 1e-15
        l32, g32 = R.bce_const(x, label, w, F32)
        assert abs(float(l32) - l.item()) < 1e-4 * max(1.0, abs(l.item())) and np.abs(g32 - tx.grad.numpy()).max() < 1e-6 * w32 / count


def test_ema_is_two_products_and_a_sum():
    s, p = F32([1.0, 0.3, -7.0]), F32([0.5, 0.1, 3.0])
    got = R.ema(s, p, 0.999)
    want = (tt(p) * float(F32(1.0 - 0.999)) + tt(s) * float(F32(0.999))).numpy()      # torch rounds each product, then the sum
    assert np.array_equal(got, want) and got.dtype == F32
    assert np.array_equal(R.ema(s, p, 0.0), p) and np.array_equal(R.ema(s, p, 1.0), s)


def test_unpacker_against_the_documented_order():
    """A block filled with its own element index: element [tap, row, k] of a plain f16 block sits at
    ((((tap * KS + ks) * mt + tile) * 2 + kh) * 32 + m) * E + e with k = (ks * 2 + kh) * E + e."""
    for dt, e in ((F32, 4), (F16, 8)):
        for mt in (1, 2):
            n = R.block_elems(mt)
            a = R.unpack_block(np.arange(n).astype(F32 if dt == F32 else np.int16), mt)
            ks_n = 32 // (2 * e)
            for tap, row, k in ((0, 0, 0), (8, 32 * mt - 1, 31), (3, 17, 9), (5, 32 * mt - 5, 16)):
                ks, kh, el = k // (2 * e), (k // e) % 2, k % e
                assert int(a[tap, row, k]) == ((((tap * ks_n + ks) * mt + row // 32) * 2 + kh) * 32 + row % 32) * e + el
    raw = (np.arange(9 * 2 * 2048) % 251).astype(np.uint8)
    m = R.unpack_mx_block(raw, 2)
    for tap, row, p, k in ((0, 0, 0, 0), (8, 63, 1, 31), (4, 33, 1, 15), (2, 7, 0, 16)):
        piece = ((tap * 2 + p) * 2 + row // 32) * 64 + (k // 16) * 32 + row % 32
        assert m[tap, row, p * 32 + k] == raw[piece * 16 + k % 16]


def test_chunk_weights_against_a_convolution():
    """The transposed, flipped chunk IS the adjoint's kernel: conv_transpose2d(g, W) == conv2d(g, W^T flipped); the virtual kernel of a
    4 x 4 stride-2 convolution gives the same output over the space-to-depth image."""
    arena, chunks, _, sv = R.pack_table()
    c = chunks[3]
    wt = R.chunk_weights(arena, c)[:, :c.m_count, :c.k_count]                           # [tap, cin, cout]
    w = tt(arena[c.src_off:c.src_off + 24 * 40 * 9].reshape(24, 40, 3, 3)).double()
    g = torch.randn(1, 24, 5, 6, dtype=torch.float64)
    want = F.conv_transpose2d(g, w, padding=1) * float(F32(0.2))
    got = F.conv2d(g, tt(wt.astype(F64)).permute(1, 2, 0).reshape(40, 24, 3, 3), padding=1)
    assert (got - want).abs().max().item() < 1e-6
    c = chunks[4]
    wv = R.chunk_weights(arena, c)[:, :16, :24]
    w4 = tt(arena[c.src_off:c.src_off + 16 * 6 * 16].reshape(16, 6, 4, 4)).double()
    x = torch.randn(1, 6, 8, 10, dtype=torch.float64)
    want = F.conv2d(x, w4, stride=2, padding=1) * sv
    xs = tt(D.s2d_ref(x.permute(0, 2, 3, 1).numpy())).permute(0, 3, 1, 2)
    got = F.conv2d(xs, tt(wv.astype(F64)).permute(1, 2, 0).reshape(16, 24, 3, 3), padding=1)
    assert (got - want).abs().max().item() < 1e-6
    w0, w1, w2 = R.exact16_blocks(F32([0.1234567]))
    assert abs((float(w0[0]) + float(w1[0])) / 4096 - float(F32(0.1234567))) < 2.0 ** -22 * 0.13 and float(w2[0]) == float(F16(float(w0[0]) / 4096))


# ---- the rule has power ------------------------------------------------------------------------------------------------------------
def rejected_bits(got, want):
    return R.bits_differ(got, want).size > 0


def trunc16(v32):
    """fp32 -> f16 by truncation: the defect 'round toward zero'."""
    r = R.f16_rne(v32)
    with np.errstate(invalid="ignore"):
        over = np.abs(r.astype(F32)) > np.abs(np.asarray(v32, dtype=F32))
    return np.where(over & np.isfinite(np.asarray(v32, dtype=F32)), np.nextafter(r, F16(0)), r).astype(F16)


def test_nchw_to_nhwc_mutations_are_rejected():
    cases = R.nchw_cases()
    hit = dict.fromkeys(["order", "trunc", "lo4096", "q_swap", "q_chunk", "prescale_twice", "mask_ignored", "pad_nonzero"], 0)
    for name, c in cases.items():
        src, mask = R.nchw_inputs(name, c)
        bits = R.AMAX_STATES.get(c["amax"])
        want = R.nchw_to_nhwc(src, c["r"], c["c_pad"], c["kind"], mask, bits, c["q"])
        for key in want:
            assert R.bits_differ(want[key], want[key].copy()).size == 0
        r, cp, kind = c["r"], c["c_pad"], c["kind"]
        if r > 1:                                                    # channel order j * r + i
            sw = R.nchw_to_nhwc(np.swapaxes(src, 2, 3), r, cp, kind, None if mask is None else np.swapaxes(mask, 2, 3), bits)["hi"]
            hit["order"] += rejected_bits(np.swapaxes(sw, 1, 2), want["hi"])
            assert rejected_bits(np.swapaxes(sw, 1, 2), want["hi"]) or src.shape[2] == r, name
        if kind != "f32":
            v = R.nchw_to_nhwc(src, r, cp, "f32", mask, bits)["hi"]
            hit["trunc"] += rejected_bits(trunc16(v), want["hi"])
        if kind == "f16x2":
            v = R.nchw_to_nhwc(src, r, cp, "f32", mask, bits)["hi"]
            with np.errstate(all="ignore"):
                lo = R.f16_rne(v - want["hi"].astype(F32))
            hit["lo4096"] += rejected_bits(lo, want["lo"])
            assert rejected_bits(lo, want["lo"]), name
        if c["q"]:
            q = want["q"]
            hit["q_swap"] += rejected_bits(np.concatenate([q[..., 32:], q[..., :32]], axis=-1), q)
            assert rejected_bits(np.concatenate([q[..., 32:], q[..., :32]], axis=-1), q), name
            if cp == 64:
                hit["q_chunk"] += rejected_bits(np.stack([q[..., 0, :], q[..., 0, :]], axis=-2), q)
            tq = q.copy()
            tq[..., 0, :32] = trunc16(v[..., :32]).view(np.uint16) >> 8   # bf8 by truncating the f16 pattern
            hit["trunc"] += rejected_bits(tq, q)
        if c["amax"] == "lifted":
            twice = R.nchw_to_nhwc(src * R.grad_prescale(bits), r, cp, kind, mask, bits)["hi"]
            hit["prescale_twice"] += rejected_bits(twice, want["hi"])
            assert rejected_bits(twice, want["hi"]), name
        if mask is not None:
            assert rejected_bits(R.nchw_to_nhwc(src, r, cp, kind, None, bits)["hi"], want["hi"]), name
            hit["mask_ignored"] += 1
        if c["c"] * r * r < cp:
            bad = want["hi"].copy()
            bad[..., -1] = -0.0                                     # a padding channel that is not +0
            hit["pad_nonzero"] += rejected_bits(bad, want["hi"])
    assert all(hit.values()), hit


def test_nhwc_to_nchw_mutations_are_rejected():
    hit = {"order": 0, "inverse_missing": 0, "lo_dropped": 0}
    for name, c in R.nhwc_cases().items():
        v32, bits = R.nhwc_loaded(name, c)[0], R.AMAX_STATES.get(c["amax"])
        want = R.nhwc_to_nchw(v32, c["c"], c["r"], bits)
        if c["r"] > 1 and c["h"] > c["r"]:
            sw = np.swapaxes(R.nhwc_to_nchw(np.swapaxes(v32, 1, 2), c["c"], c["r"], bits), 2, 3)
            assert rejected_bits(sw, want), name
            hit["order"] += 1
        if c["amax"] == "lifted":
            assert rejected_bits(R.nhwc_to_nchw(v32, c["c"], c["r"], None), want), name
            hit["inverse_missing"] += 1
        if c["kind"] == "f16x2":
            hi = R.nhwc_loaded(name, c)[1]
            assert rejected_bits(R.nhwc_to_nchw(hi.astype(F32), c["c"], c["r"], bits), want), name
            hit["lo_dropped"] += 1
    assert all(hit.values()), hit


def test_absmax_mutations_are_rejected():
    hit = {"tail": 0, "signed_max": 0, "no_backoff": 0, "no_clamp": 0, "nan_lost": 0}
    for name, c in R.absmax_cases().items():
        x = R.absmax_input(c)
        want = R.absmax_slot(x, c["t"], c["slot1"], c["slot2"])
        n = c["count"]
        if n % 4 and n > 4 and c["fill"] == "normal":
            hit["tail"] += R.absmax_slot(x[:n - n % 4], c["t"], c["slot1"], c["slot2"]) != want
        if c["fill"] == "normal":
            with np.errstate(over="ignore", under="ignore"):
                signed = float(F32(x.max()) * F32(math.ldexp(1.0, -c["t"])))
            hit["signed_max"] += want[0] != R.float_to_bits(abs(signed)) and c["slot1"] == 0 and c["slot2"] == 0
        hit["no_backoff"] += want != R.absmax_slot(x, c["t"], 0, 0) and want[0] != R.absmax_slot(x, c["t"], 0, 0)[0]
        if want[0] != "nan" and want[1] and (want[0] >> 23) == 254:
            hit["no_clamp"] += 1
        if c["fill"] == "nan":
            assert want[0] == "nan"
            hit["nan_lost"] += 1
    assert all(hit.values()), hit


def test_sumpool_mutations_are_rejected():
    hit = {"tap": 0, "mask_lo": 0, "mask_ge": 0}
    for name, c in R.sumpool_cases().items():
        xh, xl, mh, ml, pos = R.sumpool_operands(name, c)
        v32 = xh.astype(F32) if xl is None else R.pair_load32(xh, xl)
        p = pos if c["mask"] else None
        good = R.sumpool2x2(v32, p, dtype=F32)
        stored = R.store(c["kind"], good)
        val = stored["hi"].astype(F64) if c["kind"] != "f16x2" else R.pair_value(stored["hi"], stored["lo"])
        rec = R.judge_sumpool(c, val, xh, xl, pos)
        assert rec["bad"] == 0 and rec["ratio"] <= 1.0, (name, rec)
        miss = good - v32[:, 1::2, 1::2] * (np.where(pos, F32(1), F32(0.2)) if c["mask"] else F32(1))
        assert R.judge_sumpool(c, miss, xh, xl, pos)["bad"] > 0, name
        hit["tap"] += 1
        if c["mask"] and c["kind"] == "f16x2":
            wrong = R.sumpool2x2(v32, mh > 0, dtype=F32)
            assert R.judge_sumpool(c, wrong, xh, xl, pos)["bad"] > 0, name
            hit["mask_lo"] += 1
        if c["mask"] and c["kind"] != "f16x2" and mh.size >= 4:
            assert R.judge_sumpool(c, R.sumpool2x2(v32, mh >= 0, dtype=F32), xh, xl, pos)["bad"] > 0, name
            hit["mask_ge"] += 1
    assert all(hit.values()), hit


def test_add_and_ema_mutations_are_rejected():
    rng = np.random.default_rng(5)
    for e, dt in ((4, F32), (8, F16)):
        for k in R.ADD_COUNTS_E:
            a, b = rng.standard_normal(k * e).astype(dt), rng.standard_normal(k * e).astype(dt)
            want = R.add_plain(a, b)
            assert rejected_bits(np.concatenate([want[:-e], a[-e:]]), want)          # the last 16 bytes never added
            if dt == F16:
                assert rejected_bits(trunc16(a.astype(F32) + b.astype(F32)), want) or k == 1
    for k in R.ADD_COUNTS_E:
        ah, al = R.pair_split(rng.standard_normal(k * 8).astype(F32))
        bh, bl = R.pair_split(rng.standard_normal(k * 8).astype(F32))
        ref64 = R.pair_value(ah, al) + R.pair_value(bh, bl)
        v32 = R.add_pair32(ah, al, bh, bl)
        s = R.store("f16x2", v32)
        assert R.judge(R.pair_value(s["hi"], s["lo"]), ref64, v32, "pair")["bad"] == 0
        nolo = R.store("f16x2", ah.astype(F32) + bh.astype(F32))
        assert R.judge(R.pair_value(nolo["hi"], nolo["lo"]), ref64, v32, "pair")["bad"] > 0      # the lo halves never added
        hi16 = R.f16_rne(v32)
        assert R.judge(hi16.astype(F64), ref64, v32, "pair")["bad"] > 0                          # the sum stored as one f16
    for count in R.EMA_COUNTS[:5]:
        s, p = rng.standard_normal(count).astype(F32), rng.standard_normal(count).astype(F32)
        want = R.ema(s, p, 0.999)
        fused = (F64(F32(1.0 - 0.999)) * p.astype(F64) + (F32(0.999) * s).astype(F64)).astype(F32)        # one product kept exact: an fma
        if count >= 100:
            assert rejected_bits(fused, want)
        if count % 4:
            assert rejected_bits(np.concatenate([want[:count - count % 4], s[count - count % 4:]]), want)   # a dropped count % 4 tail


def test_loss_mutations_are_rejected():
    w = 0.37
    for count in R.LOSS_COUNTS[:-1]:
        a, b, x = R.loss_inputs(count)
        l64, g64 = R.l1_mean(a, b, w)
        l32, g32 = R.l1_mean(a, b, w, F32)
        assert R.judge(l32, l64, l32, "f32")["bad"] == 0
        assert rejected_bits(R.l1_mean(a, b, w, F32, sign0=1.0)[1], g32)                      # sign(0) = 1
        if count % 4 and count > 4:
            k = count - count % 4
            tail_less = R.seq_sum32(np.abs(a[:k] - b[:k])) * R.gscale32(w, count)
            assert R.judge(tail_less, l64, l32, "f32")["bad"] > 0, count
        for label in (0.0, 1.0):
            l64, g64 = R.bce_const(x, label, w)
            l32, g32 = R.bce_const(x, label, w, F32)
            ge, le = R.bce_exp_terms(x, w)
            assert R.judge(g32, g64, g32, "f32", ge)["bad"] == 0 and R.judge(l32, l64, l32, "f32", le)["bad"] == 0
            if label:
                nolabel = R.bce_const(x, 0.0, w, F32)[1]
                assert R.judge(nolabel, g64, g32, "f32", ge)["bad"] > 0                       # a gradient without the label
            if count % 4 and count > 4:
                k = count - count % 4
                gt = g32.copy()
                gt[k:] = np.nan                                                               # never written: the output's NaN pre-fill stays
                assert R.judge(gt, g64, g32, "f32", ge)["bad"] > 0, count
    # the exp term is small against what it excuses: at |x| = 100 it is 102 * 2^-24 of s (1 - s) ~ e^-100
    ge, _ = R.bce_exp_terms(F32([0.0, 100.0]), 1.0)
    assert ge[0] == 0.5 * 0.25 * 2 * 2.0 ** -24 and ge[1] < 1e-45


def test_pack_mutations_are_rejected():
    arena, chunks, elems, sv = R.pack_table()
    seen = {"flip": 0, "unscaled_w1": 0, "zero_fill": 0}
    for ch in chunks:
        for kind in R.DTYPES:
            want = R.expected_blocks(arena, ch, kind)
            if ch.transposed:
                assert rejected_bits(R.expected_blocks(arena, ch, kind, flip=False)[0], want[0])
                seen["flip"] += 1
            if kind == "f16x2" and (ch.scale != 1.0 or ch.scale_value is not None):
                assert rejected_bits(R.expected_blocks(arena, ch, kind, unscaled_w1=True)[1], want[1])
                seen["unscaled_w1"] += 1
            if ch.m_count < 32 * ch.mt or ch.k_count < 32:
                assert not want[0][:, ch.m_count:, :].any() and not want[0][:, :, ch.k_count:].any()
                seen["zero_fill"] += 1
        both = (R.expected_blocks(arena, ch, "f16")[0], R.expected_f16_fused(arena, ch))
        for ev in both:                                              # either legal evaluation of a plain f16 block passes, a wrong one does not
            assert R.f16_block_differs(ev, arena, ch)[0].size == 0
        if ch.transposed:
            assert R.f16_block_differs(R.expected_blocks(arena, ch, "f16", flip=False)[0], arena, ch)[0].size > 0
        assert R.f16_block_differs(np.nextafter(both[0], F16(np.inf)), arena, ch)[0].size > 0       # one f16 ulp off everywhere
        mx = R.expected_mx(arena, ch)
        assert rejected_bits(np.concatenate([mx[..., 32:], mx[..., :32]], axis=2), mx)
    assert all(seen.values()), seen
    assert {c.mt for c in chunks} == {1, 2} and any(c.virtual4x4 for c in chunks) and any(c.scale_value is not None for c in chunks)
