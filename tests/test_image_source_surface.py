"""CPU: the host side of the whole-image data source -- `device_data.reflect101` against numpy's reflect padding, the definition
`crop_sample_np` against `augment_np` on a numpy-padded image, the draws of `sample_crop_draw`, what `check_crop_records` refuses, the
declaration and the argument checks of resr_crop_batch, `config.data_source` = images / images_loader with `config.train_tile`, and
`dataset.CropImageDataset`.  Every comparison is bit for bit."""
import ctypes as C
import importlib
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def D():
    import __graft_entry__
    __graft_entry__.build()
    from real_esrgan_pytorch_amd import device_data
    return device_data


def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- the definition --------------------------------------------------------------------------------------------------------------
def test_reflect101_is_numpys_reflect_padding_for_any_pad_width(D):
    for n in range(1, 9):
        axis = np.arange(n)
        for pad in range(0, 40):
            want = np.pad(axis, (0, pad), mode="reflect")              # pads larger than n - 1 included: numpy reflects again
            assert [D.reflect101(i, n) for i in range(n + pad)] == want.tolist(), (n, pad)
    for i, n in ((-1, 4), (0, 0)):
        with pytest.raises(ValueError, match="reflect101"):
            D.reflect101(i, n)


def test_crop_sample_np_on_a_tile_is_augment_np_for_every_code(D):
    for T in (5, 6):                                                    # odd; even: the zero row / column of 90 / 180 / 270
        tile = _image(T, T, T)
        for code in range(16):
            got = D.crop_sample_np(tile, 0, 0, code, T)
            assert torch.is_tensor(got) and got.dtype == torch.float32 and tuple(got.shape) == (3, T, T)
            assert _same_bits(got.numpy(), D.augment_np(tile, code).numpy()), (T, code)


@pytest.mark.parametrize("T", [1, 4, 7])
def test_crop_sample_np_is_augment_np_of_the_padded_images_window(D, T):
    """Images smaller than, equal to and larger than T in either axis, every corner window and one inside, codes running through all 16."""
    sizes = [(1, 1), (1, 9), (2, 3), (T, T), (max(1, T - 1), T + 5), (T + 5, max(1, T - 1)), (3 * T + 1, 2 * T + 7), (T, 2 * T)]
    code = 0
    for k, (h, w) in enumerate(sizes):
        image = _image(h, w, 10 * T + k)
        hp, wp = max(h, T), max(w, T)
        padded = np.pad(image, ((0, hp - h), (0, wp - w), (0, 0)), mode="reflect")
        assert padded.shape[:2] == (hp, wp) and np.array_equal(padded[:h, :w], image)
        for top, left in {(0, 0), (0, wp - T), (hp - T, 0), (hp - T, wp - T), ((hp - T) // 2, (wp - T + 1) // 2)}:
            for _ in range(4):
                got = D.crop_sample_np(image, top, left, code, T)
                want = D.augment_np(np.ascontiguousarray(padded[top:top + T, left:left + T]), code)
                assert _same_bits(got.numpy(), want.numpy()), (h, w, top, left, code)
                code = (code + 5) % 16
        for top, left in ((hp - T + 1, 0), (0, wp - T + 1), (-1, 0), (0, -1)):      # a window never starts past the legal range
            with pytest.raises(ValueError, match="crop_sample_np: the"):
                D.crop_sample_np(image, top, left, 0, T)
    with pytest.raises(ValueError, match="uint8"):
        D.crop_sample_np(_image(4, 4, 0).astype(np.float32), 0, 0, 0, T)
    with pytest.raises(ValueError, match="code"):
        D.crop_sample_np(_image(T, T, 0), 0, 0, 16, T)
    with pytest.raises(ValueError, match="below 1"):
        D.crop_sample_np(_image(4, 4, 0), 0, 0, 0, 0)


def test_sample_crop_draw_draws_only_for_an_axis_above_the_window(D):
    T = 8
    for seed in range(16):
        np_before, torch_before = np.random.get_state(), torch.get_rng_state()
        for h, w in ((8, 8), (3, 8), (8, 1), (5, 7)):                   # both sides <= T: no draw at all
            random.seed(seed)
            start = random.getstate()
            assert D.sample_crop_draw(h, w, T) == (0, 0) and random.getstate() == start, (h, w)
        for h, w, draws in ((37, 20, ("top", "left")), (37, 8, ("top",)), (6, 20, ("left",)), (9, 9, ("top", "left"))):
            random.seed(seed)
            top, left = D.sample_crop_draw(h, w, T)
            after = random.getstate()
            random.seed(seed)                                           # the replay: the same calls, typed out
            want_top = random.randint(0, h - T) if "top" in draws else 0
            want_left = random.randint(0, w - T) if "left" in draws else 0
            assert random.getstate() == after, (seed, h, w)              # exactly these draws, no more
            assert (top, left) == (want_top, want_left) and 0 <= top <= max(h, T) - T and 0 <= left <= max(w, T) - T
        now = np.random.get_state()
        assert now[0] == np_before[0] and np.array_equal(now[1], np_before[1]) and now[2:] == np_before[2:]
        assert torch.equal(torch.get_rng_state(), torch_before)


def test_check_crop_records_refuses_each_bad_field_by_name(D):
    table = np.asarray([[0, 10, 12], [360, 3, 20], [540, 8, 8]], dtype=np.int64)      # T = 8: image 1 is padded below
    ok = np.asarray([[0, 2, 4, 15], [1, 0, 12, 0], [2, 0, 0, 5]], dtype=np.int32)
    out = D.check_crop_records(ok, table, 8)
    assert out.dtype == np.int32 and out.shape == (3, 4) and np.array_equal(out, ok)
    for bad, word in (([3, 0, 0, 0], "image index 3"), ([-1, 0, 0, 0], "image index -1"), ([0, 3, 0, 0], "top 3"), ([0, -1, 0, 0], "top -1"),
                      ([0, 0, 5, 0], "left 5"), ([0, 0, -2, 0], "left -2"), ([1, 1, 0, 0], "top 1"), ([1, 0, 13, 0], "left 13"),
                      ([2, 1, 0, 0], "top 1"), ([2, 0, 1, 0], "left 1"), ([0, 0, 0, 16], "code 16"), ([0, 0, 0, -1], "code -1")):
        rec = ok.copy()
        rec[1] = bad
        with pytest.raises(ValueError, match=f"crop records: {word} of record 1"):
            D.check_crop_records(rec, table, 8)
    with pytest.raises(ValueError, match="crop records: expected integer"):
        D.check_crop_records(np.zeros((2, 3), np.int32), table, 8)
    with pytest.raises(ValueError, match="crop records: expected integer"):
        D.check_crop_records(np.zeros((1, 4), np.float32), table, 8)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_once_and_the_library_exports_it(D):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert len(re.findall(r"\bint resr_crop_batch\(", text)) == 1
    assert "resr_crop_batch" in _lib.exported_symbols()
    res, args = _lib._PROTOS["resr_crop_batch"]
    assert res is C.c_int and len(args) == 8
    assert callable(C.CDLL(_lib.LIB_PATH).resr_crop_batch)              # the built library itself, not the binding's table
    assert callable(_lib.lib().resr_crop_batch)


def test_crop_batch_answers_every_bad_argument_before_any_launch(D):
    """No device is touched: the checks come first, and a call that got as far as a launch would not return RESR_ERR_ARG.  The pointers
    are never dereferenced on the host."""
    from real_esrgan_pytorch_amd import _lib
    one = C.c_void_p(8)
    ok = dict(arena=one, table=one, records=one, m=1, b=1, t=4, dst=one)
    cases = [(dict(arena=None), b"null pointer"), (dict(table=None), b"null pointer"), (dict(records=None), b"null pointer"),
             (dict(dst=None), b"null pointer"),
             (dict(m=0), b"m=0"), (dict(m=-1), b"m=-1"), (dict(b=0), b"b=0"), (dict(b=-2), b"b=-2"), (dict(t=0), b"t=0"), (dict(t=-4), b"t=-4"),
             (dict(b=65536), b"b=65536 above 65535"),
             (dict(t=2 ** 31 - 1), b"grid overflow"), (dict(t=32 * 46341), b"grid overflow")]      # 46341^2 is the first square >= 2^31
    for change, word in cases:
        a = dict(ok, **change)
        rc = _lib.lib().resr_crop_batch(a["arena"], a["table"], a["records"], a["m"], a["b"], a["t"], a["dst"], None)
        text = _lib.lib().resr_last_error()
        assert rc == _lib.RESR_ERR_ARG and b"crop_batch" in text and word in text, (change, rc, text)
    assert 46340 ** 2 < 2 ** 31 <= 46341 ** 2


# ---- config ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def config(D, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(source=None, tile=None, mode=None):
        for name, value in (("RESR_DATA_SOURCE", source), ("RESR_TRAIN_TILE", tile), ("RESR_MODE", mode), ("RESR_PAIRED_LR_DIR", None)):
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


def test_config_takes_both_image_sources_and_checks_the_window(config, monkeypatch):
    for source in ("images", "images_loader"):
        c = config(source)
        assert c.data_source == source and source in c.DATA_SOURCES and source in c.IMAGE_DATA_SOURCES
        assert c.train_tile == 400 and c.train_window() == 400          # upstream's crop_pad_size
        assert config(source, "256").train_window() == 256              # the window may be exactly image_size
        for mode in ("train_realesrnet", "train_realesrgan"):
            with pytest.raises(ValueError, match="train_tile=255.*RESR_TRAIN_TILE.*image_size=256"):
                config(source, "255", mode)
        assert config(source, "255", "test").train_tile == 255          # not a training mode: nothing to check
    c = config()                                                        # the default is untouched
    assert c.data_source == "loader" and c.train_tile == 400
    assert config("loader", "8").train_tile == 8 and config("device", "8").data_source == "device"      # the other sources never read it
    with pytest.raises(ValueError, match="RESR_DATA_SOURCE") as info:
        config("hbm")
    assert all(repr(name) in str(info.value) for name in ("loader", "device", "paired", "paired_loader", "images", "images_loader"))
    c = config("images")
    monkeypatch.setattr(c, "image_size", 401)
    with pytest.raises(ValueError, match="train_tile=400.*image_size=401"):
        c.train_window()


# ---- the loader path ---------------------------------------------------------------------------------------------------------------
def test_crop_image_dataset_yields_the_definition_for_a_seeded_draw(D, tmp_path):
    from PIL import Image
    from real_esrgan_pytorch_amd import config as cfg
    from real_esrgan_pytorch_amd.dataset import CropImageDataset
    T = 16
    folder = tmp_path / "images"
    folder.mkdir()
    for k, (w, h) in enumerate(((7, 5), (30, 38), (64, 64))):           # below T in both axes; above in both; well above
        Image.fromarray(_image(h, w, k)).save(str(folder / f"{k}.png"))
    data = CropImageDataset(str(folder), T, cfg.degradation_model_parameters_dict)
    names = os.listdir(str(folder))
    assert len(data) == 3 and [os.path.basename(p) for p in data.image_file_names] == names
    for i, name in enumerate(names):
        image = np.asarray(Image.open(str(folder / name)).convert("RGB"))
        random.seed(40 + i)
        np.random.seed(40 + i)
        top, left = D.sample_crop_draw(image.shape[0], image.shape[1], T)      # the sample's draws, in its order
        code = D.sample_augment()
        records = D.sample_blur_params(cfg.degradation_model_parameters_dict)
        after = random.getstate(), np.random.get_state()
        assert (image.shape[0] > T) == (name != "0.png") and 0 <= top <= max(image.shape[0], T) - T and 0 <= left <= max(image.shape[1], T) - T
        random.seed(40 + i)
        np.random.seed(40 + i)
        item = data[i]
        assert random.getstate() == after[0] and np.array_equal(np.random.get_state()[1], after[1][1])      # these draws and nothing else
        assert set(item) == {"hr", "kernel1", "kernel2", "sinc_kernel"} and all(v.dtype == torch.float32 for v in item.values())
        assert item["hr"].shape == (3, T, T) and all(item[n].shape == (21, 21) for n in ("kernel1", "kernel2", "sinc_kernel"))
        assert _same_bits(item["hr"].numpy(), D.crop_sample_np(image, top, left, code, T).numpy()), name
        kernels = D.blur_kernels_from_params_np(records)
        for n, want in zip(("kernel1", "kernel2", "sinc_kernel"), kernels):
            assert _same_bits(item[n].numpy(), want), (name, n)
    with pytest.raises(ValueError, match="tile 0"):
        CropImageDataset(str(folder), 0, cfg.degradation_model_parameters_dict)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no files"):
        CropImageDataset(str(tmp_path / "empty"), T, cfg.degradation_model_parameters_dict)


def test_from_dir_refuses_bad_sets_before_any_device_work(D, tmp_path):
    from PIL import Image
    dev = torch.device("cuda", 0)      # never reached: every refusal below comes first
    folder = tmp_path / "set"
    folder.mkdir()
    for k, (w, h) in enumerate(((7, 5), (9, 12))):
        Image.fromarray(_image(h, w, k)).save(str(folder / f"{k}.png"))
    total = (7 * 5 + 9 * 12) * 3
    with pytest.raises(ValueError, match=f"{total} bytes, above max_bytes={total - 1}"):
        D.ImageCropSource.from_dir(str(folder), 1, 8, dev, max_bytes=total - 1)
    with pytest.raises(ValueError, match="tile 0"):
        D.ImageCropSource.from_dir(str(folder), 1, 0, dev)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no files"):
        D.ImageCropSource.from_dir(str(tmp_path / "empty"), 1, 8, dev)
    with pytest.raises(ValueError, match="max_bytes"):
        D.ImageCropSource.from_arrays([_image(4, 4, 0)], 1, 8, dev, max_bytes=47)
    with pytest.raises(ValueError, match="image 1 must be uint8"):
        D.ImageCropSource.from_arrays([_image(4, 4, 0), _image(4, 4, 0).astype(np.float32)], 1, 8, dev)
    with pytest.raises(ValueError, match="no images"):
        D.ImageCropSource.from_arrays([], 1, 8, dev)
