"""-m gpu: resr_crop_batch against its definition, device_data.crop_sample_np, bit for bit -- there is no tolerance: the kernel moves
bytes and divides by 255.0f, as the definition does.  The shapes are the smallest that can go wrong: window sides below, at and across
the 32-pixel tile with a ragged last tile, odd and even (the zero row / column of a rotation), images below, at and above the window in
either axis -- so blocks wholly inside the image, blocks that cross into the padding and pads wider than the image --, every corner
window, all 16 codes, an arena with odd offsets, one image past byte 2^31, and records the kernel has to clamp."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gpu_util

pytestmark = pytest.mark.gpu

CROP_BATCH_ID = 33003
BATCH = 3


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


def _launches(L, fn):
    """(kernel id, bytes) of every launch inside fn()."""
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 64))
    return [(buf[i].kernel_id, buf[i].bytes) for i in range(n)]


def _arena(images, front=1):
    """The images behind `front` bytes with 1, 2, 3, 1, ... bytes between them (0xEE: a byte the images' neighbours must never show);
    returns (bytes, table [M,3])."""
    parts, rows, at = [np.full(front, 0xEE, np.uint8)], [], front
    for k, a in enumerate(images):
        rows.append((at, a.shape[0], a.shape[1]))
        gap = 1 + k % 3
        parts += [a.reshape(-1), np.full(gap, 0xEE, np.uint8)]
        at += a.size + gap
    return np.concatenate(parts), np.asarray(rows, dtype=np.int64)


def _case(T):
    """The images of the sweep and, for each, every legal corner window plus one inside, each under all 16 codes."""
    sizes = []
    for h, w in ((1, 1), (1, 9), (2, 3), (T, T), (T - 1, T + 5), (T + 5, T - 1), (3 * T + 1, 2 * T + 7), (70, 45)):
        if h > 0 and w > 0 and (h, w) not in sizes:
            sizes.append((h, w))
    rng = np.random.default_rng(T)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    records = []
    for i, (h, w) in enumerate(sizes):
        tm, lm = max(h, T) - T, max(w, T) - T
        for top, left in sorted({(0, 0), (0, lm), (tm, 0), (tm, lm), (tm // 2, (lm + 1) // 2)}):
            records += [(i, top, left, code) for code in range(16)]
    return images, np.asarray(records, dtype=np.int32)


def _same_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (what, bad.size, np.unravel_index(bad[0], want.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("T", [1, 2, 3, 5, 8, 31, 32, 33, 67])
def test_crop_batch_is_crop_sample_np_bit_for_bit(D, L, T):
    images, records = _case(T)
    arena, table = _arena(images)
    assert any(int(o) % 2 for o in table[:, 0]) and any(int(o) % 4 for o in table[:, 0])      # images start at unaligned bytes
    assert D.check_crop_records(records, table, T) is not None and set(records[:, 3].tolist()) == set(range(16))
    a_dev, t_dev = gpu_util.dev(arena), gpu_util.dev(table)
    groups = -(-records.shape[0] // BATCH)
    for g in range(groups):                                             # launch g: records g, g + groups, g + 2 groups -- other images, other codes
        rec = records[[(g + k * groups) % records.shape[0] for k in range(BATCH)]]
        want = np.stack([D.crop_sample_np(images[i], top, left, code, T).numpy() for i, top, left, code in rec.tolist()])
        out = gpu_util.Out(want.size, np.float32)                       # guard words on both sides of dst
        r_dev = gpu_util.dev(rec)
        seen = _launches(L, lambda: L.check(L.lib().resr_crop_batch(L.ptr(a_dev), L.ptr(t_dev), L.ptr(r_dev), len(images), BATCH, T,
                                                                    C.c_void_p(out.ptr), L.stream_ptr()), "resr_crop_batch"))
        assert seen == [(CROP_BATCH_ID, BATCH * T * T * 15.0)], seen    # ONE launch, under its profiling id and byte count
        _same_bits(out.read().reshape(want.shape), want, (T, rec.tolist()))      # (read(): every element written, no guard touched)
        if g == 0:                                                      # the Python wrapper, the same bits
            got = D.crop_batch(a_dev, t_dev, r_dev, T)
            torch.cuda.synchronize()
            _same_bits(got.cpu().numpy(), want, "wrapper")


def test_crop_batch_reads_an_image_past_2_31_bytes(D):
    """An arena above 2^31 bytes (a real set's is): the last image starts at an odd offset past the reach of a 32-bit one, and is below
    the window in one axis.  The arena is allocated as zeros on the device; no host array of that size is made."""
    T = 33
    rng = np.random.default_rng(7)
    images = [np.zeros((40, 50, 3), np.uint8), rng.integers(1, 256, (37, 20, 3), dtype=np.uint8)]      # image 0: the zeros of the arena
    far = 2 ** 31 + 1
    arena = torch.zeros(far + images[1].size, dtype=torch.uint8, device="cuda")
    arena[far:] = gpu_util.dev(images[1].reshape(-1))
    table = np.asarray([(0, 40, 50), (far, 37, 20)], dtype=np.int64)
    records = np.asarray([(1, 4, 0, 0), (0, 2, 7, 3), (1, 0, 0, 6), (1, 1, 0, 13)], dtype=np.int32)
    assert D.check_crop_records(records, table, T) is not None
    want = np.stack([D.crop_sample_np(images[i], top, left, code, T).numpy() for i, top, left, code in records.tolist()])
    got = D.crop_batch(arena, gpu_util.dev(table), gpu_util.dev(records), T)
    torch.cuda.synchronize()
    _same_bits(got.cpu().numpy(), want, "far image")
    assert float(got[1].abs().max()) == 0.0 and float(got[0].min()) > 0.0


def test_crop_batch_clamps_a_wrong_record_into_its_image(D, L):
    """Nothing of a record is trusted on the device: image into 0..M-1, top / left into the legal range of that image, the code's low four
    bits.  The answer is the clamped record's; no error, and nothing around dst is written."""
    T = 8
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((12, 10), (5, 20), (8, 8))]
    arena, table = _arena(images)
    big, small = 2 ** 31 - 1, -2 ** 31
    cases = [((-3, 1, 1, 2), (0, 1, 1, 2)), ((7, 0, 0, 9), (2, 0, 0, 9)), ((big, 0, 5, 1), (2, 0, 0, 1)), ((small, 4, 2, 0), (0, 4, 2, 0)),
             ((0, -5, 1, 4), (0, 0, 1, 4)), ((0, 100, 1, 7), (0, 4, 1, 7)), ((0, big, small, 3), (0, 4, 0, 3)),
             ((1, 1, 3, 5), (1, 0, 3, 5)), ((1, 0, 1000, 6), (1, 0, 12, 6)), ((1, small, big, 10), (1, 0, 12, 10)),
             ((2, 1, 1, 11), (2, 0, 0, 11)), ((0, 2, 2, 16 + 5), (0, 2, 2, 5)), ((0, 2, 2, -1), (0, 2, 2, 15)), ((1, 0, 4, 0x7FFFFFF0 + 6), (1, 0, 4, 6))]
    assert len(cases) % BATCH != 0                                      # the last launch is shorter: B = 2
    a_dev, t_dev = gpu_util.dev(arena), gpu_util.dev(table)
    for start in range(0, len(cases), BATCH):
        chunk = cases[start:start + BATCH]
        sent = np.asarray([c[0] for c in chunk], dtype=np.int64).astype(np.int32)
        clamped = np.asarray([c[1] for c in chunk], dtype=np.int32)
        with pytest.raises(ValueError, match="crop records"):           # the host check is what refuses such a record
            D.check_crop_records(sent, table, T)
        assert D.check_crop_records(clamped, table, T) is not None
        want = np.stack([D.crop_sample_np(images[i], top, left, code, T).numpy() for i, top, left, code in clamped.tolist()])
        out = gpu_util.Out(want.size, np.float32)
        r_dev = gpu_util.dev(sent)
        L.check(L.lib().resr_crop_batch(L.ptr(a_dev), L.ptr(t_dev), L.ptr(r_dev), len(images), len(chunk), T, C.c_void_p(out.ptr), L.stream_ptr()),
                "resr_crop_batch")
        _same_bits(out.read().reshape(want.shape), want, sent.tolist())


def test_crop_batch_refusals_come_before_any_launch(D, L):
    arena = torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    table = gpu_util.dev(np.asarray([(0, 4, 4)], dtype=np.int64))
    records = gpu_util.dev(np.zeros((2, 4), dtype=np.int32))
    out = gpu_util.Out(2 * 3 * 4 * 4, np.float32)
    ok = dict(arena=L.ptr(arena), table=L.ptr(table), records=L.ptr(records), m=1, b=2, t=4, dst=C.c_void_p(out.ptr))
    cases = [(dict(arena=None), b"null pointer"), (dict(table=None), b"null pointer"), (dict(records=None), b"null pointer"), (dict(dst=None), b"null pointer"),
             (dict(m=0), b"m=0"), (dict(m=-1), b"m=-1"), (dict(b=0), b"b=0"), (dict(b=-2), b"b=-2"), (dict(t=0), b"t=0"), (dict(t=-4), b"t=-4"),
             (dict(b=65536), b"above 65535"), (dict(t=2 ** 31 - 1), b"grid overflow"), (dict(t=32 * 46341), b"grid overflow")]

    def call(a):
        return L.lib().resr_crop_batch(a["arena"], a["table"], a["records"], a["m"], a["b"], a["t"], a["dst"], L.stream_ptr())
    answers = []

    def refused():
        for change, word in cases:
            answers.append((change, word, call(dict(ok, **change)), L.lib().resr_last_error()))
    seen = _launches(L, refused)
    for change, word, rc, text in answers:
        assert rc == L.RESR_ERR_ARG and b"crop_batch" in text and word in text, (change, rc, text)
    assert len(answers) == len(cases) and seen == []                    # no profiling record: nothing was launched
    out.read(written=False)
    assert (out.t.view(torch.int32) == out._sent()).all()
    assert _launches(L, lambda: L.check(call(ok), "resr_crop_batch")) == [(CROP_BATCH_ID, 2 * 4 * 4 * 15.0)]      # the arguments the cases start from do run
    out.read()
    for args in ((arena.float(), table, records), (arena.view(4, -1), table, records), (arena, table.int(), records), (arena, table, records.long()),
                 (arena, table.view(-1), records), (arena, table, records.view(-1))):
        with pytest.raises(ValueError, match="crop_batch"):
            D.crop_batch(*args, 4)
    with pytest.raises(ValueError, match="crop_batch"):
        D.crop_batch(arena, table, records, 0)
    with pytest.raises(ValueError, match="crop_batch: out"):
        D.crop_batch(arena, table, records, 4, out=torch.empty(2, 3, 4, 5, device="cuda"))
