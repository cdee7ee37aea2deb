"""-m gpu: resr_resample_u8 against its definition, device_data.resample_u8_np, bit for bit -- there is no tolerance: both are the same
integer rule (tests/test_multiscale_surface.py holds the definition to Pillow itself and the library's tables to the definition's).

Every case lays its images out in one arena filled with 0xEE: sources and destinations at bytes of every alignment with 1, 2, 3 guard bytes
between them, and the WHOLE arena is compared after the launch -- the destinations are the definition's bytes, and no source and no guard
byte has changed.  The sizes are the smallest that can go wrong: sides 1 .. 101 in both axes under the three scales, two short sides and an
enlargement (outputs below, at and across the 64 x 16 tile, up to 4 x 9 tiles), an unchanged axis, rows of 1801 and 2101 taps (more rows and
columns than one staged chunk, coefficient rows too long for LDS), a job past byte 2^31, tables with wrong bounds, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gpu_util

pytestmark = pytest.mark.gpu

RESAMPLE_ID = 33004
FILL = 0xEE
SIDES = (1, 2, 3, 5, 17, 33, 64, 67, 101)
SCALES = (0.75, 0.5, 1 / 3)


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


def _layout(shapes, front=1):
    """(h, w, oh, ow) per job -> (arena bytes, [(source offset, h, w, destination offset, oh, ow)]): all sources, then all destinations, 1, 2,
    3, 1, ... guard bytes between neighbours."""
    at, pairs = front, []
    for k, (h, w, _, _) in enumerate(shapes):
        pairs.append([at, h, w])
        at += h * w * 3 + 1 + k % 3
    for k, (_, _, oh, ow) in enumerate(shapes):
        pairs[k] += [at, oh, ow]
        at += oh * ow * 3 + 1 + (k + 1) % 3
    return at, [tuple(p) for p in pairs]


def _arena(shapes, seed):
    """The host arena (0xEE, the sources random bytes or 0 / 255 checkerboards) and its pairs."""
    size, pairs = _layout(shapes)
    arena = np.full(size, FILL, np.uint8)
    rng = np.random.default_rng(seed)
    for k, (src, h, w, _, _, _) in enumerate(pairs):
        if k % 4 == 3:
            y, x = np.mgrid[0:h, 0:w]
            image = np.stack([((y + x + c) % 2) * 255 for c in range(3)], axis=2).astype(np.uint8)
        else:
            image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        arena[src:src + h * w * 3] = image.reshape(-1)
    return arena, pairs


def _expected(D, arena, pairs, cache, tables_of=None):
    """The arena after the launch: every destination the definition's resample of its source, everything else as it was."""
    want = arena.copy()
    for j, (src, h, w, dst, oh, ow) in enumerate(pairs):
        for pair in ((h, oh), (w, ow)):
            if pair[0] != pair[1] and pair not in cache:
                cache[pair] = D.resample_tables_np(*pair)
        tables = tables_of(j) if tables_of else (cache.get((h, oh)), cache.get((w, ow)))
        image = arena[src:src + h * w * 3].reshape(h, w, 3)
        want[dst:dst + oh * ow * 3] = D.resample_u8_np(image, oh, ow, tables=tables).reshape(-1)
    return want


def _run(L, a_dev, jobs, tables_dev):
    jobs_dev = gpu_util.dev(jobs)
    return lambda: L.check(L.lib().resr_resample_u8(L.ptr(a_dev), int(a_dev.numel()), jobs.ctypes.data, L.ptr(jobs_dev), int(jobs.shape[0]), L.ptr(tables_dev),
                                                    int(tables_dev.numel()), L.stream_ptr()), "resr_resample_u8")


def _same_arena(got, want, pairs):
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0])
        owner = [j for j, (_, _, _, dst, oh, ow) in enumerate(pairs) if dst <= at < dst + oh * ow * 3]
        raise AssertionError(f"{bad.size} bytes differ, first at {at}: got {got[at]}, want {want[at]}; " +
                             (f"destination of job {owner[0]} {pairs[owner[0]]}" if owner else "a source or guard byte was written"))


@pytest.fixture(scope="module")
def table_cache():
    return {}


def _size_set(D):
    out = []
    for i, h in enumerate(SIDES):
        for step in (0, 2, 5):
            w = SIDES[(i + step) % len(SIDES)]
            sizes = D.multiscale_sizes(h, w, SCALES, 4) + D.multiscale_sizes(h, w, (), 40) + [(h + h // 3 + 1, 2 * w + 1)]
            out += [(h, w, oh, ow) for oh, ow in sizes]
    return out


def test_one_launch_of_many_jobs_is_the_definition_bit_for_bit(D, L, table_cache):
    shapes = _size_set(D) + [(33, 17, 33, 8), (33, 17, 11, 17), (5, 5, 5, 5), (130, 260, 97, 195)]      # + an unchanged axis (both: a copy), 4 x 7 tiles
    arena, pairs = _arena(shapes, 1)
    assert {src % 4 for src, *_ in pairs} == {0, 1, 2, 3} and {(dst + y * ow * 3) % 4 for _, _, _, dst, oh, ow in pairs for y in range(oh)} == {0, 1, 2, 3}
    assert max(ow for *_, ow in pairs) > 3 * 64 and max(oh for *_, oh, _ in pairs) > 8 * 16
    jobs, tables = D.resample_jobs(pairs)
    assert jobs.shape == (len(shapes), 8) and jobs.dtype == np.int64 and tables.dtype == np.int32
    want = _expected(D, arena, pairs, table_cache)
    a_dev, t_dev = gpu_util.dev(arena), gpu_util.dev(tables)
    seen = _launches(L, _run(L, a_dev, jobs, t_dev))
    moved = float(sum(h * w * 3 + oh * ow * 3 for _, h, w, _, oh, ow in pairs))
    assert seen == [(RESAMPLE_ID, moved)], seen                        # ONE launch, under its profiling id, the bytes read and written in its record
    _same_arena(a_dev.cpu().numpy(), want, pairs)
    b_dev = gpu_util.dev(arena)                                        # the Python wrapper, uploading the jobs itself: the same bytes
    assert D.resample_u8(b_dev, jobs, t_dev) is b_dev
    torch.cuda.synchronize()
    _same_arena(b_dev.cpu().numpy(), want, pairs)


def test_rows_longer_than_a_chunk_and_than_the_staged_taps(D, L, table_cache):
    """300 -> 1 rows (1801 taps: 19 row chunks), 700 -> 2 columns (2101 taps: 3 source chunks, coefficients read from the table), both at
    once, and 41 taps (one above the staged 40)."""
    shapes = [(300, 7, 1, 3), (5, 700, 4, 2), (300, 700, 2, 3), (9, 410, 9, 61), (20, 200, 40, 150)]
    assert [D.resample_ksize(300, 1), D.resample_ksize(700, 2), D.resample_ksize(410, 61)] == [1801, 2101, 43]
    arena, pairs = _arena(shapes, 2)
    jobs, tables = D.resample_jobs(pairs)
    want = _expected(D, arena, pairs, table_cache)
    a_dev = gpu_util.dev(arena)
    D.resample_u8(a_dev, jobs, gpu_util.dev(tables))
    torch.cuda.synchronize()
    _same_arena(a_dev.cpu().numpy(), want, pairs)


def test_a_job_past_byte_2_31(D, L, table_cache):
    """An arena above 2^31 bytes (a real set's is): source and destination both start past the reach of a 32-bit offset, at odd bytes.  The
    arena is allocated on the device; no host array of that size is made."""
    far = 2 ** 31 + 1
    shapes = [(67, 101, 50, 75), (40, 50, 13, 16)]
    small, pairs = _arena(shapes, 3)
    a_dev = torch.full((far + small.size,), FILL, dtype=torch.uint8, device="cuda")
    a_dev[far:] = gpu_util.dev(small)
    moved = [(src + far, h, w, dst + far, oh, ow) for src, h, w, dst, oh, ow in pairs]
    jobs, tables = D.resample_jobs(moved)
    assert a_dev.numel() > 2.1e9 and (jobs[:, 0] > 2 ** 31).all() and (jobs[:, 3] > 2 ** 31).all()
    want = _expected(D, small, pairs, table_cache)
    D.resample_u8(a_dev, jobs, gpu_util.dev(tables))
    torch.cuda.synchronize()
    _same_arena(a_dev[far:].cpu().numpy(), want, pairs)
    assert bool((a_dev[far - 4096:far] == FILL).all()) and bool((a_dev[:4096] == FILL).all())


def test_wrong_bounds_are_clamped_into_the_source(D, L, table_cache):
    """Nothing read from a table is trusted for addressing: xmin is clamped into 0 .. in - 1 and count into 0 .. min(ksize, in - xmin), the
    definition's clamp.  The answer is the clamped table's; no source and no guard byte changes."""
    shapes = [(33, 67, 24, 50), (17, 5, 12, 3), (64, 64, 21, 21), (101, 33, 40, 13)]
    arena, pairs = _arena(shapes, 4)
    jobs, tables = D.resample_jobs(pairs)
    big, small = 2 ** 31 - 1, -2 ** 31
    wrong = [(-5, 3), (big, 2), (small, big), (0, -1), (0, 0), (3, big), (1, small), (big, big), (2, 5000), (-1, -1), (7, 1)]
    used = {}
    for j, (_, h, w, _, oh, ow) in enumerate(pairs):
        both = []
        for n, out, at in ((h, oh, int(jobs[j, 6])), (w, ow, int(jobs[j, 7]))):
            ksize = D.resample_ksize(n, out)
            bounds = tables[at:at + 2 * out].reshape(out, 2)           # a view: the upload below carries the wrong bounds
            for row in range(out):
                if (row + j) % 3:
                    bounds[row] = wrong[(row * 7 + j) % len(wrong)]
            both.append((bounds.copy(), tables[at + 2 * out:at + out * (2 + ksize)].reshape(out, ksize).copy()))
        used[j] = tuple(both)
    want = _expected(D, arena, pairs, table_cache, tables_of=lambda j: used[j])
    assert not np.array_equal(want, _expected(D, arena, pairs, table_cache))      # the wrong bounds do change the answer
    a_dev = gpu_util.dev(arena)
    D.resample_u8(a_dev, jobs, gpu_util.dev(tables))
    torch.cuda.synchronize()
    _same_arena(a_dev.cpu().numpy(), want, pairs)


def test_refusals_come_before_any_launch(D, L):
    shapes = [(8, 12, 4, 6), (5, 5, 5, 5)]
    arena, pairs = _arena(shapes, 5)
    jobs, tables = D.resample_jobs(pairs)
    a_dev, t_dev, j_dev = gpu_util.dev(arena), gpu_util.dev(tables), gpu_util.dev(jobs)

    def call(change=None, **args):
        host = jobs.copy()
        for (row, column), value in (change or {}).items():
            host[row, column] = value
        a = dict(dict(arena=L.ptr(a_dev), arena_bytes=int(a_dev.numel()), host=host.ctypes.data, dev=L.ptr(j_dev), j=2, tables=L.ptr(t_dev),
                      words=int(t_dev.numel())), **args)
        return L.lib().resr_resample_u8(a["arena"], a["arena_bytes"], a["host"], a["dev"], a["j"], a["tables"], a["words"], L.stream_ptr())
    src0, dst0, dst1 = pairs[0][0], pairs[0][3], pairs[1][3]
    cases = [(dict(arena=None), b"null pointer"), (dict(host=None), b"null pointer"), (dict(dev=None), b"null pointer"), (dict(tables=None), b"null pointer"),
             (dict(j=0), b"j=0"), (dict(j=65536), b"j=65536 outside 1..65535"),
             (dict(change={(0, 1): 0}), b"below 1 or at or above 2^31"), (dict(change={(1, 5): 2 ** 31}), b"below 1 or at or above 2^31"),
             (dict(change={(0, 1): 8000, (0, 4): 1}), b"outside 1..4096"), (dict(words=int(t_dev.numel()) - 1), b"leaves the table buffer"),
             (dict(arena_bytes=dst1 + 74), b"leaves the arena"),
             (dict(change={(0, 3): src0 + 1}), b"overlapping source and destination"), (dict(change={(1, 3): dst0 + 71}), b"overlapping source and destination"),
             (dict(change={(1, 0): dst0}), b"overlapping source and destination")]
    answers = []

    def refused():
        for args, word in cases:
            answers.append((args, word, call(**args), L.lib().resr_last_error()))
    seen = _launches(L, refused)
    for args, word, rc, text in answers:
        assert rc == L.RESR_ERR_ARG and b"resample_u8" in text and word in text, (args, rc, text)
    assert len(answers) == len(cases) and seen == []                    # no profiling record: nothing was launched
    torch.cuda.synchronize()
    assert np.array_equal(a_dev.cpu().numpy(), arena)                   # and nothing was written
    assert [k for k, _ in _launches(L, lambda: L.check(call(), "resr_resample_u8"))] == [RESAMPLE_ID]      # the arguments the cases start from do run
    for args in ((a_dev.float(), jobs, t_dev), (a_dev[:8].view(2, 4), jobs, t_dev), (a_dev, jobs.astype(np.int32), t_dev), (a_dev, jobs.reshape(-1), t_dev),
                 (a_dev, j_dev, t_dev), (a_dev, jobs, t_dev.float()), (a_dev, jobs, t_dev.cpu())):
        with pytest.raises(ValueError, match="resample_u8"):
            D.resample_u8(*args)
    with pytest.raises(ValueError, match="resample_u8: jobs_dev"):
        D.resample_u8(a_dev, jobs, t_dev, jobs_dev=j_dev[:1])
