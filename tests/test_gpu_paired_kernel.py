"""-m gpu: resr_pair_batch against its definition, device_data.paired_sample_np, bit for bit -- there is no tolerance: the kernel moves
bytes and divides by 255.0f, as the definition does.  The shapes are the smallest that can go wrong: patch sides below, at and across
the 32-pixel tile with a ragged last tile, every scale, all 8 codes, images of exactly the patch, row lengths that leave every row
unaligned, crops in the four corners, arenas with odd offsets, and one image past byte 2^31.

Only legal records reach the GPU here: the kernel's clamp of a record is a safety net that stays unexercised, and what refuses a wrong
record, device_data.check_paired_records, is tested on the CPU (tests/test_paired_surface.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gpu_util

pytestmark = pytest.mark.gpu

PAIR_BATCH_ID = 33001


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


def _launch_ids(L, fn):
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 64))
    return [buf[i].kernel_id for i in range(n)]


def _arena(images, front, gap):
    """The images back to back behind `front` bytes, `gap` bytes between them (0xEE: a byte the images' neighbours must never show);
    returns (bytes, offsets)."""
    parts, offsets, at = [np.full(front, 0xEE, np.uint8)], [], front
    for a in images:
        offsets.append(at)
        parts += [a.reshape(-1), np.full(gap, 0xEE, np.uint8)]
        at += a.size + gap
    return np.concatenate(parts), offsets


def _case(patch, scale):
    """Images (lr h, w): one of exactly the patch, one a little larger, and one per row length 7 / 33 / 70 that holds the patch.  Records:
    the patch-sized image under all 8 codes (its only crop is (0, 0)), every other image at its four corners -- the last legal top and
    left among them -- and once inside, the codes running on."""
    P = patch
    sizes = [(P, P), (P + 4, P + 2)] + [(P + 1, w) for w in (7, 33, 70) if w >= P]
    rng = np.random.default_rng(100 * P + scale)
    lr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    hr = [rng.integers(0, 256, (scale * h, scale * w, 3), dtype=np.uint8) for h, w in sizes]
    records = [(0, 0, 0, code) for code in range(8)]
    for i, (h, w) in enumerate(sizes[1:], start=1):
        for top, left in ((0, 0), (0, w - P), (h - P, 0), (h - P, w - P), ((h - P) // 2, (w - P + 1) // 2)):
            records.append((i, top, left, (3 * len(records) + 1) % 8))
    return hr, lr, np.asarray(records, dtype=np.int32)


def _want(D, hr, lr, records, patch, scale):
    pairs = [D.paired_sample_np(hr[i], lr[i], top, left, code, patch, scale) for i, top, left, code in records.tolist()]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _same_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
@pytest.mark.parametrize("patch", [1, 5, 32, 33, 67])
def test_pair_batch_is_paired_sample_np_bit_for_bit(D, L, patch, scale):
    hr, lr, records = _case(patch, scale)
    B = records.shape[0]
    assert set(records[:, 3].tolist()) == set(range(8)) and D.check_paired_records(records, [(0, 0) + a.shape[:2] for a in lr], patch) is not None
    want_lr, want_hr = _want(D, hr, lr, records, patch, scale)
    hr_bytes, hr_off = _arena(hr, front=3, gap=1)                       # odd offsets on both sides
    lr_bytes, lr_off = _arena(lr, front=1, gap=2)
    assert any(o % 2 for o in hr_off) and any(o % 2 for o in lr_off)
    table = np.asarray([(ho, lo) + a.shape[:2] for ho, lo, a in zip(hr_off, lr_off, lr)], dtype=np.int64)
    h_dev, l_dev, t_dev, r_dev = gpu_util.dev(hr_bytes), gpu_util.dev(lr_bytes), gpu_util.dev(table), gpu_util.dev(records)
    out_lr, out_hr = gpu_util.Out(want_lr.size, np.float32), gpu_util.Out(want_hr.size, np.float32)
    ids = _launch_ids(L, lambda: L.check(L.lib().resr_pair_batch(L.ptr(h_dev), L.ptr(l_dev), L.ptr(t_dev), L.ptr(r_dev), len(lr), B, patch, scale,
                                                                   C.c_void_p(out_lr.ptr), C.c_void_p(out_hr.ptr), L.stream_ptr()), "resr_pair_batch"))
    assert ids == [PAIR_BATCH_ID], ids                                  # ONE launch writes both outputs, under its profiling id
    _same_bits(out_lr.read().reshape(want_lr.shape), want_lr, "lr")     # (read(): every element written, no guard touched)
    _same_bits(out_hr.read().reshape(want_hr.shape), want_hr, "hr")
    if patch in (5, 33):                                                # the Python wrapper, the same bits
        got_lr, got_hr = D.pair_batch(h_dev, l_dev, t_dev, r_dev, patch, scale)
        torch.cuda.synchronize()
        _same_bits(got_lr.cpu().numpy(), want_lr, "wrapper lr")
        _same_bits(got_hr.cpu().numpy(), want_hr, "wrapper hr")


def test_pair_batch_reads_an_image_past_2_31_bytes(D):
    """An HR arena above 2^31 bytes (a real set's is): the second image starts at an odd offset past the reach of a 32-bit one.  The
    arena is allocated as zeros on the device; no host array of that size is made."""
    patch, scale = 33, 2
    rng = np.random.default_rng(7)
    lr = [rng.integers(1, 256, (35, 40, 3), dtype=np.uint8), rng.integers(1, 256, (34, 37, 3), dtype=np.uint8)]
    hr = [np.zeros((70, 80, 3), np.uint8), rng.integers(1, 256, (68, 74, 3), dtype=np.uint8)]      # image 0's HR side: the zeros of the arena
    far = 2 ** 31 + 1
    hr_arena = torch.zeros(far + hr[1].size, dtype=torch.uint8, device="cuda")
    hr_arena[far:] = gpu_util.dev(hr[1].reshape(-1))
    lr_bytes, lr_off = _arena(lr, front=0, gap=0)
    table = np.asarray([(0, lr_off[0], 35, 40), (far, lr_off[1], 34, 37)], dtype=np.int64)
    records = np.asarray([(1, 1, 4, 0), (0, 2, 7, 3), (1, 0, 0, 6), (1, 1, 4, 5)], dtype=np.int32)
    want_lr, want_hr = _want(D, hr, lr, records, patch, scale)
    got_lr, got_hr = D.pair_batch(hr_arena, gpu_util.dev(lr_bytes), gpu_util.dev(table), gpu_util.dev(records), patch, scale)
    torch.cuda.synchronize()
    _same_bits(got_lr.cpu().numpy(), want_lr, "lr")
    _same_bits(got_hr.cpu().numpy(), want_hr, "hr")
    assert float(got_hr[1].abs().max()) == 0.0 and float(got_hr[0].min()) > 0.0


def test_pair_batch_refusals_come_before_any_launch(D, L):
    hr, lr = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device="cuda"), torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    table = gpu_util.dev(np.asarray([(0, 0, 4, 4)], dtype=np.int64))
    records = gpu_util.dev(np.zeros((2, 4), dtype=np.int32))
    out_lr, out_hr = gpu_util.Out(2 * 3 * 4 * 4, np.float32), gpu_util.Out(2 * 3 * 16 * 16, np.float32)
    ok = dict(hr=L.ptr(hr), lr=L.ptr(lr), table=L.ptr(table), records=L.ptr(records), m=1, b=2, patch=4, scale=4, lr_dst=C.c_void_p(out_lr.ptr),
              hr_dst=C.c_void_p(out_hr.ptr))
    cases = [dict(hr=None), dict(lr=None), dict(table=None), dict(records=None), dict(lr_dst=None), dict(hr_dst=None),
             dict(m=0), dict(m=-1), dict(b=0), dict(b=-2), dict(patch=0), dict(patch=-4), dict(scale=0), dict(scale=5), dict(scale=-1),
             dict(b=65536),                                              # the grid's y dimension
             dict(patch=2 ** 31 - 1, scale=2), dict(patch=2 ** 30, scale=4),   # scale * patch above 2^31 - 1
             dict(patch=2 ** 31 - 1, scale=1), dict(patch=2 ** 21, scale=1), dict(patch=2 ** 19, scale=4)]   # that fits, the tile count does not

    def call(a):
        return L.lib().resr_pair_batch(a["hr"], a["lr"], a["table"], a["records"], a["m"], a["b"], a["patch"], a["scale"], a["lr_dst"], a["hr_dst"],
                                       L.stream_ptr())
    answers = []

    def refused():
        for change in cases:
            answers.append((change, call(dict(ok, **change)), L.lib().resr_last_error()))
    ids = _launch_ids(L, refused)
    for change, rc, text in answers:
        assert rc == L.RESR_ERR_ARG and b"pair_batch" in text, (change, rc, text)
    assert len(answers) == len(cases) and ids == []                     # no profiling record: nothing was launched
    out_lr.read(written=False)
    out_hr.read(written=False)
    assert (out_lr.t.view(torch.int32) == out_lr._sent()).all() and (out_hr.t.view(torch.int32) == out_hr._sent()).all()
    L.check(call(ok), "resr_pair_batch")                                # the arguments the cases start from do run
    out_lr.read()
    out_hr.read()
    h1 = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for args in ((h1.float(), lr, table, records), (hr, lr.view(4, -1), table, records), (hr, lr, table.int(), records), (hr, lr, table, records.long()),
                 (hr, lr, table.view(-1), records)):
        with pytest.raises(ValueError, match="pair_batch"):
            D.pair_batch(*args, 4, 4)
