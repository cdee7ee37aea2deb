"""CPU: the host side of the multi-scale copies of the whole-image data source -- the definition `device_data.resample_tables_np` /
`resample_u8_np` against Pillow itself (`Image.resize(..., LANCZOS)`, Pillow 12.2.0 when this was written; the test prints the installed
version), the library's host table builder against the definition as integers, the declarations and the refusals of the three new
entries (none of them reaches a launch), `multiscale_sizes`, the table rule of `ImageCropSource`, `config.train_copies()` and the loader twin
`dataset.CropImageDataset` with copies.  Every comparison is bit for bit."""
import ctypes as C
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (1, 2, 3, 5, 17, 33, 64, 67, 101)
SCALES = (0.75, 0.5, 1 / 3)
BIG_PAIRS = ((2040, 1530), (2040, 680), (1356, 400))


@pytest.fixture(scope="module")
def D():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import device_data
    return device_data


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _checkerboard(h, w):
    """0 / 255 squares of one pixel, the three channels out of phase: the negative lobes clip at both ends."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((y + x + c) % 2) * 255 for c in range(3)], axis=2).astype(np.uint8)


def _cases(D):
    """(h, w, oh, ow): every side of SIDES in both axes (each h with three w), the copies `multiscale_sizes` gives for the scales and for the
    short sides 4 and 40, and one enlarging size."""
    out = []
    for i, h in enumerate(SIDES):
        for step in (0, 2, 5):
            w = SIDES[(i + step) % len(SIDES)]
            sizes = D.multiscale_sizes(h, w, SCALES, 4) + D.multiscale_sizes(h, w, (), 40) + [(h + h // 3 + 1, 2 * w + 1)]
            out += [(h, w, oh, ow) for oh, ow in sizes]
    return out


@pytest.fixture(scope="module")
def tables(D):
    """resample_tables_np of every (in, out) pair the cases need, made once."""
    made = {}
    for h, w, oh, ow in _cases(D):
        for pair in ((h, oh), (w, ow)):
            if pair[0] != pair[1] and pair not in made:
                made[pair] = D.resample_tables_np(*pair)
    return made


def _resample(D, tables, image, oh, ow):
    h, w = image.shape[:2]
    return D.resample_u8_np(image, oh, ow, tables=(tables.get((h, oh)), tables.get((w, ow))))


# ---- the definition against Pillow ---------------------------------------------------------------------------------------------------
def test_resample_u8_np_is_pillows_lanczos_resize_bit_for_bit(D, tables):
    """Pillow 12.2.0 on the machine this was written on."""
    import PIL
    from PIL import Image
    print("Pillow", PIL.__version__)
    cases = _cases(D)
    assert len(cases) == 27 * 6 and any(oh > h and ow > w for h, w, oh, ow in cases) and any(oh == h or ow == w for h, w, oh, ow in cases)
    for n, (h, w, oh, ow) in enumerate(cases):
        for image in (_image(h, w, n), _checkerboard(h, w)):
            want = np.asarray(Image.fromarray(image).resize((ow, oh), Image.LANCZOS))
            got = _resample(D, tables, image, oh, ow)
            assert got.dtype == np.uint8 and got.shape == (oh, ow, 3) and np.array_equal(got, want), (h, w, oh, ow)
    lo, hi = _resample(D, tables, _checkerboard(101, 67), 75, 50), _resample(D, tables, _checkerboard(64, 101), 85, 203)
    assert lo.min() == 0 or hi.min() == 0
    assert hi.max() == 255                                             # the clip is reached
    with pytest.raises(ValueError, match="resample_u8_np: expected a uint8"):
        D.resample_u8_np(_image(4, 4, 0).astype(np.float32), 2, 2)
    with pytest.raises(ValueError, match="below 1"):
        D.resample_u8_np(_image(4, 4, 0), 0, 2)


def test_the_definition_without_given_tables_and_with_an_unchanged_axis(D):
    from PIL import Image
    image = _image(33, 17, 3)
    for oh, ow in ((33, 17), (33, 8), (11, 17), (24, 12)):
        assert np.array_equal(D.resample_u8_np(image, oh, ow), np.asarray(Image.fromarray(image).resize((ow, oh), Image.LANCZOS))), (oh, ow)
    assert D.resample_u8_np(image, 33, 17) is not image


def test_multiscale_sizes_are_upstreams_arithmetic(D):
    assert D.multiscale_sizes(1356, 2040, SCALES, 400) == [(1017, 1530), (678, 1020), (452, 680), (400, int(400 * (2040 / 1356)))]
    assert D.multiscale_sizes(2040, 1356, (), 400) == [(int(400 * (2040 / 1356)), 400)]
    assert D.multiscale_sizes(5, 5, (0.5,), 7) == [(2, 2), (7, 7)] and D.multiscale_sizes(1, 2, (1 / 3, 0.75)) == [(1, 1), (1, 1)]
    assert D.multiscale_sizes(9, 9) == []


# ---- the host table builder ------------------------------------------------------------------------------------------------------------
def test_native_tables_equal_the_definition_as_integers(D, tables):
    pairs = sorted(tables) + list(BIG_PAIRS) + [(100, 1), (33, 67), (7, 2), (3, 1)]
    worst = 0
    for n, out in pairs:
        bounds, coeffs = tables[(n, out)] if (n, out) in tables else D.resample_tables_np(n, out)
        got_bounds, got_coeffs = D.resample_tables(n, out)
        assert got_bounds.dtype == got_coeffs.dtype == np.int32 and coeffs.shape == (out, D.resample_ksize(n, out))
        assert np.array_equal(got_bounds, bounds) and np.array_equal(got_coeffs, coeffs), (n, out)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n).all() and (bounds[:, 1] >= 1).all()
        worst = max(worst, int(np.abs(coeffs.astype(np.int64)).sum(axis=1).max()))
    assert 255 * worst + 2 ** 21 < 2 ** 31 and worst < 1.6 * 2 ** 22      # the int32 accumulator has room
    assert D.resample_ksize(2040, 400) == 33 and D.resample_ksize(33, 67) == 7 and D.resample_ksize(100, 1) == 601


def test_header_declares_the_entries_once_and_the_library_exports_them(D):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    for name, count in (("resr_resample_ksize", 2), ("resr_resample_tables", 5), ("resr_resample_u8", 8)):
        assert len(re.findall(rf"\bint {name}\(", text)) == 1
        assert name in _lib.exported_symbols() and len(_lib._PROTOS[name][1]) == count
        assert callable(getattr(C.CDLL(_lib.LIB_PATH), name)) and callable(getattr(_lib.lib(), name))


def test_table_builder_refusals(D):
    from real_esrgan_pytorch_amd import _lib
    lib = _lib.lib()
    bounds, coeffs = np.zeros((4, 2), np.int32), np.zeros((4, 16), np.int32)
    ok = dict(n=8, out=4, bounds=bounds.ctypes.data, coeffs=coeffs.ctypes.data, cap=16)
    assert D.resample_ksize(8, 4) == 13
    for change, word in ((dict(n=0), b"in_size=0"), (dict(out=0), b"out_size=0"), (dict(n=-3), b"in_size=-3"), (dict(n=2 ** 31), b"outside 1..2^31 - 1"),
                         (dict(bounds=None), b"null pointer"), (dict(coeffs=None), b"null pointer"), (dict(cap=12), b"ksize_capacity=12 below the 13 taps")):
        a = dict(ok, **change)
        rc = lib.resr_resample_tables(a["n"], a["out"], a["bounds"], a["coeffs"], a["cap"])
        text = lib.resr_last_error()
        assert rc == _lib.RESR_ERR_ARG and b"resample" in text and word in text, (change, rc, text)
    assert lib.resr_resample_ksize(0, 4) == _lib.RESR_ERR_ARG and lib.resr_resample_ksize(4, 2 ** 31) == _lib.RESR_ERR_ARG
    assert not bounds.any() and not coeffs.any()                       # a refusal writes nothing
    assert lib.resr_resample_tables(8, 4, bounds.ctypes.data, coeffs.ctypes.data, 16) == 0      # a capacity above ksize: the rows' stride
    want_bounds, want_coeffs = D.resample_tables_np(8, 4)
    assert np.array_equal(bounds, want_bounds) and np.array_equal(coeffs[:, :13], want_coeffs) and not coeffs[:, 13:].any()
    # (the accumulator refusal, 255 * sum|coeff| + 2^21 >= 2^31, cannot be reached with this filter: the test above bounds sum|coeff| instead)
    with pytest.raises(ValueError, match="below 1"):
        D.resample_tables_np(0, 1)


def test_resample_u8_answers_every_bad_argument_before_any_launch(D):
    """No device is touched: the checks come first and read only the host copy of the jobs; the other pointers are never dereferenced."""
    from real_esrgan_pytorch_amd import _lib
    one = C.c_void_p(8)
    words = 4 * (2 + 13) + 6 * (2 + 13)
    good = [0, 8, 12, 1000, 4, 6, 0, 4 * (2 + 13), 288, 5, 5, 2000, 5, 5, 0, 0]      # 8x12 -> 4x6 with both tables; 5x5 copied
    assert D.resample_ksize(8, 4) == 13 and D.resample_ksize(12, 6) == 13

    def call(jobs, arena=one, arena_bytes=4096, host=True, dev=one, j=None, tables=one, table_words=None):
        a = np.asarray(jobs, dtype=np.int64).reshape(-1, 8)
        return _lib.lib().resr_resample_u8(arena, arena_bytes, a.ctypes.data if host else None, dev, a.shape[0] if j is None else j, tables,
                                           words if table_words is None else table_words, None)

    def job(**change):
        fields = dict(src=0, h=8, w=12, dst=1000, oh=4, ow=6, rows=0, cols=4 * (2 + 13))
        fields.update(change)
        return [fields[k] for k in ("src", "h", "w", "dst", "oh", "ow", "rows", "cols")]
    cases = [(lambda: call(good, arena=None), b"null pointer"), (lambda: call(good, host=False), b"null pointer"), (lambda: call(good, dev=None), b"null pointer"),
             (lambda: call(good, tables=None), b"null pointer"), (lambda: call(good, j=0), b"j=0"), (lambda: call(good, j=-1), b"j=-1"),
             (lambda: call(good, j=65536), b"j=65536 outside 1..65535"), (lambda: call(good, arena_bytes=0), b"arena_bytes=0"),
             (lambda: call(job(h=0)), b"below 1 or at or above 2^31"), (lambda: call(job(ow=0)), b"below 1 or at or above 2^31"),
             (lambda: call(job(w=2 ** 31)), b"below 1 or at or above 2^31"), (lambda: call(job(oh=-4)), b"below 1 or at or above 2^31"),
             (lambda: call(job(h=2000, oh=1, src=0, dst=2000 * 12 * 3), arena_bytes=10 ** 6, table_words=10 ** 6), b"ksize=12001 of 2000 -> 1 outside 1..4096"),
             (lambda: call(job(cols=words - 10)), b"column table at word"), (lambda: call(job(rows=-1)), b"row table at word"),
             (lambda: call(job(), table_words=words - 1), b"leaves the table buffer"),
             (lambda: call(job(src=-1)), b"leaves the arena"), (lambda: call(job(dst=4096 - 71)), b"leaves the arena"), (lambda: call(job(src=4096 - 287)), b"leaves the arena"),
             (lambda: call(job(dst=287)), b"overlapping source and destination"), (lambda: call(job(src=50, dst=0)), b"overlapping source and destination"),
             (lambda: call(job() + job(src=300, dst=1071)), b"overlapping source and destination"),            # two destinations share a byte
             (lambda: call(job() + job(src=1000, dst=2000)), b"overlapping source and destination")]           # a source is another job's destination
    for k, (run, word) in enumerate(cases):
        rc = run()
        text = _lib.lib().resr_last_error()
        assert rc == _lib.RESR_ERR_ARG and b"resample_u8" in text and word in text, (k, rc, text)
    with pytest.raises(RuntimeError, match="resample_u8: expected a tensor on the MI355X"):      # the wrapper has no CPU path
        D.resample_u8(torch.zeros(8, dtype=torch.uint8), np.zeros((1, 8), np.int64), torch.zeros(4, dtype=torch.int32))


# ---- the table of the source -------------------------------------------------------------------------------------------------------------
def test_crop_table_keeps_the_originals_first_and_puts_copy_k_of_image_i_at_row_m_1_k_i(D):
    sizes = [(30, 41), (8, 8), (101, 3)]
    names = ["a", "b", "c"]
    plain = D._crop_table(sizes, names, 10 ** 9)
    table = D._crop_table(sizes, names, 10 ** 9, (0.75, 1 / 3), 40)
    M = 3
    assert plain.shape == (3, 3) and table.shape == (M * 4, 3) and np.array_equal(table[:M], plain)      # rows 0..M-1: today's table
    for i, (h, w) in enumerate(sizes):
        copies = D.multiscale_sizes(h, w, (0.75, 1 / 3), 40)
        assert len(copies) == 3
        for k, size in enumerate(copies):
            assert tuple(table[M * (1 + k) + i, 1:]) == size, (i, k)
    ends = table[:, 0] + table[:, 1] * table[:, 2] * 3
    assert table[0, 0] == 0 and np.array_equal(table[1:, 0], ends[:-1])      # back to back, in row order
    total = int(ends[-1])
    dev = torch.device("cuda", 0)      # never reached: every refusal below comes before any device work
    images = [_image(h, w, k) for k, (h, w) in enumerate(sizes)]
    with pytest.raises(ValueError, match=f"3 images and their 3 copies each are {total} bytes, above max_bytes={total - 1}"):
        D.ImageCropSource.from_arrays(images, 1, 8, dev, max_bytes=total - 1, scales=(0.75, 1 / 3), short_side=40)
    for scales, word in (((0.5, 1.0), "scale 1.0"), ((0.0,), "scale 0.0"), ((-0.5,), "scale -0.5"), ((float("nan"),), "scale nan"), ((float("inf"),), "scale inf"),
                         ((1.5,), "scale 1.5")):
        with pytest.raises(ValueError, match=f"train_scales: {word} is not a finite number in \\(0, 1\\)"):
            D.ImageCropSource.from_arrays(images, 1, 8, dev, scales=scales)
    with pytest.raises(ValueError, match="train_short_side=-1 is negative"):
        D.ImageCropSource.from_arrays(images, 1, 8, dev, short_side=-1)


def test_from_dir_checks_the_budget_with_the_copies_before_any_device_work(D, tmp_path):
    from PIL import Image
    folder = tmp_path / "set"
    folder.mkdir()
    for k, (w, h) in enumerate(((7, 5), (9, 12))):
        Image.fromarray(_image(h, w, k)).save(str(folder / f"{k}.png"))
    total = (7 * 5 + 9 * 12 + 3 * 2 + 4 * 6) * 3
    dev = torch.device("cuda", 0)      # never reached
    with pytest.raises(ValueError, match=f"{total} bytes, above max_bytes={total - 1}"):
        D.ImageCropSource.from_dir(str(folder), 1, 8, dev, max_bytes=total - 1, scales=(0.5,))
    with pytest.raises(ValueError, match="train_scales: scale 1.0"):
        D.ImageCropSource.from_dir(str(folder), 1, 8, dev, scales=(1.0,))


# ---- config ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def config(D, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(scales=None, short_side=None, source=None, mode=None):
        for name, value in (("RESR_TRAIN_SCALES", scales), ("RESR_TRAIN_SHORT_SIDE", short_side), ("RESR_DATA_SOURCE", source), ("RESR_MODE", mode),
                            ("RESR_TRAIN_TILE", None), ("RESR_PAIRED_LR_DIR", None)):
            monkeypatch.delenv(name, raising=False)
            if value is not None:
                monkeypatch.setenv(name, value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_config_train_copies_parses_and_refuses(config, monkeypatch):
    c = config()
    assert c.train_scales == "" and c.train_short_side == 0 and c.train_copies() == ((), 0)      # the default: no copies
    assert c.DATA_SOURCES == ("loader", "device", "paired", "paired_loader", "images", "images_loader")
    c = config("0.75, 0.5,1/3", "400", "images")
    assert c.train_copies() == ((0.75, 0.5, 1 / 3), 400)
    assert config("3/4").train_copies() == ((0.75,), 0) and config(None, "400").train_copies() == ((), 400)
    for text, word in (("1", "scale 1.0"), ("0.5,2", "scale 2.0"), ("0", "scale 0.0"), ("-1/2", "scale -0.5"), ("nan", "scale nan"), ("1/0", "neither a number nor a/b"),
                       ("half", "neither a number nor a/b"), ("1/2/3", "neither a number nor a/b")):
        c = config(text)                                                # not an image source in a training mode: nothing is checked at import
        with pytest.raises(ValueError, match=word):
            c.train_copies()
        for mode in ("train_realesrnet", "train_realesrgan"):
            for source in ("images", "images_loader"):
                with pytest.raises(ValueError, match=word):
                    config(text, None, source, mode)
        assert config(text, None, "device", "train_realesrnet").train_scales == text      # the other sources never read it
    with pytest.raises(ValueError, match="train_short_side=-5 is negative"):
        config(None, "-5").train_copies()
    c = config()
    monkeypatch.setattr(c, "train_scales", (0.5, 0.25))                 # set from code: a sequence of numbers
    monkeypatch.setattr(c, "train_short_side", 40)
    assert c.train_copies() == ((0.5, 0.25), 40)
    monkeypatch.setattr(c, "train_scales", (0.5, 1))
    with pytest.raises(ValueError, match="scale 1.0"):
        c.train_copies()


# ---- the loader twin -------------------------------------------------------------------------------------------------------------------
def test_crop_image_dataset_hands_out_windows_of_pillows_copies(D, tmp_path):
    from PIL import Image
    from real_esrgan_pytorch_amd import config as cfg
    from real_esrgan_pytorch_amd.dataset import CropImageDataset
    T, scales, short = 16, (0.75, 1 / 3), 20
    folder = tmp_path / "images"
    folder.mkdir()
    for k, (w, h) in enumerate(((7, 5), (30, 38), (64, 61))):
        Image.fromarray(_image(h, w, k)).save(str(folder / f"{k}.png"))
    plain = CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict)
    data = CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict, scales, short)
    names = os.listdir(str(folder))
    M = 3
    assert len(plain) == M and len(data) == M * 4 and data.image_file_names == plain.image_file_names
    assert len(CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict, short_side=short)) == 2 * M
    for j in range(len(data)):
        original = Image.open(str(folder / names[j % M])).convert("RGB")
        image = np.asarray(original)
        if j >= M:
            oh, ow = D.multiscale_sizes(image.shape[0], image.shape[1], scales, short)[j // M - 1]
            image = np.asarray(original.resize((ow, oh), Image.LANCZOS))
            assert np.array_equal(image, D.resample_u8_np(np.asarray(original), oh, ow))
        random.seed(70 + j)
        np.random.seed(70 + j)
        top, left = D.sample_crop_draw(image.shape[0], image.shape[1], T)      # the sample's draws, in its order
        code = D.sample_augment()
        D.sample_blur_params(cfg.degradation_model_parameters_dict)
        after = random.getstate(), np.random.get_state()
        random.seed(70 + j)
        np.random.seed(70 + j)
        item = data[j]
        assert random.getstate() == after[0] and np.array_equal(np.random.get_state()[1], after[1][1])      # these draws and nothing else
        want = D.crop_sample_np(image, top, left, code, T).numpy()
        assert item["hr"].dtype == torch.float32 and np.array_equal(item["hr"].numpy().view(np.int32), want.view(np.int32)), j
        if j < M:                                                       # unchanged below M: the dataset without copies gives the same item
            random.seed(70 + j)
            np.random.seed(70 + j)
            same = plain[j]
            assert all(torch.equal(item[k], same[k]) for k in ("hr", "kernel1", "kernel2", "sinc_kernel"))
    with pytest.raises(ValueError, match="scale 1.0"):
        CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict, (1.0,))
    with pytest.raises(ValueError, match="negative"):
        CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict, (), -2)
