"""CPU: the host side of the paired data source -- the definition `device_data.paired_sample_np` against an independent restatement,
the draws of `sample_paired_draw`, what `check_paired_records` and `PairedDeviceSource.from_dirs` refuse before a device is touched, the
declaration of resr_pair_batch, `config.data_source` = paired / paired_loader, and `dataset.PairedImageDataset`."""
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


def _pair(h, w, scale, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (scale * h, scale * w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _restated(image, top, left, side, code):
    """out[c, y, x] by indexing alone: the transpose swaps (y, x), the vertical flip mirrors the row, the horizontal flip the column."""
    out = np.empty((3, side, side), dtype=np.float32)
    for y in range(side):
        for x in range(side):
            r, c = (x, y) if code & 4 else (y, x)
            if code & 2:
                r = side - 1 - r
            if code & 1:
                c = side - 1 - c
            for ch in range(3):
                out[ch, y, x] = np.float32(image[top + r, left + c, ch]) / np.float32(255)
    return out


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_paired_sample_np_is_the_restatement_for_every_code(D, scale):
    h, w, P, top, left = 9, 11, 5, 3, 6
    hr, lr = _pair(h, w, scale, scale)
    seen = set()
    for code in range(8):
        got_lr, got_hr = D.paired_sample_np(hr, lr, top, left, code, P, scale)
        assert got_lr.dtype == np.float32 and got_lr.shape == (3, P, P) and got_lr.flags["C_CONTIGUOUS"]
        assert got_hr.dtype == np.float32 and got_hr.shape == (3, scale * P, scale * P) and got_hr.flags["C_CONTIGUOUS"]
        assert np.array_equal(got_lr.view(np.int32), _restated(lr, top, left, P, code).view(np.int32)), code
        assert np.array_equal(got_hr.view(np.int32), _restated(hr, scale * top, scale * left, scale * P, code).view(np.int32)), code
        seen.add(got_lr.tobytes())
    assert len(seen) == 8                                              # the eight codes are eight different images


def test_the_hr_crop_is_the_scale_times_block_of_the_lr_crop(D):
    """With an HR side that repeats every LR pixel scale x scale times, the HR output is the LR output repeated -- under every code."""
    lr = np.random.default_rng(2).integers(0, 256, (8, 13, 3), dtype=np.uint8)
    for scale in (2, 3, 4):
        hr = np.repeat(np.repeat(lr, scale, axis=0), scale, axis=1)
        for code in range(8):
            got_lr, got_hr = D.paired_sample_np(hr, lr, 1, 7, code, 6, scale)
            assert np.array_equal(got_hr, np.repeat(np.repeat(got_lr, scale, axis=1), scale, axis=2)), (scale, code)


def test_paired_sample_np_refuses_what_the_definition_excludes(D):
    hr, lr = _pair(8, 8, 2, 0)
    D.paired_sample_np(hr, lr, 3, 3, 7, 5, 2)                          # the last legal top / left
    for args, word in (((hr, lr, 4, 0, 0, 5, 2), "crop"), ((hr, lr, 0, -1, 0, 5, 2), "crop"), ((hr, lr, 0, 0, 8, 5, 2), "code"),
                       ((hr, lr, 0, 0, 0, 5, 5), "scale"), ((hr, lr, 0, 0, 0, 5, 4), "not 4 x"), ((hr.astype(np.float32), lr, 0, 0, 0, 5, 2), "uint8")):
        with pytest.raises(ValueError, match=word):
            D.paired_sample_np(*args)


def test_sample_paired_draw_makes_five_draws_of_random_in_the_stated_order(D):
    codes = set()
    for seed in range(64):
        random.seed(seed)
        start = random.getstate()
        np_before, torch_before = np.random.get_state(), torch.get_rng_state()
        top, left, code = D.sample_paired_draw(37, 20, 8)
        after = random.getstate()
        random.setstate(start)                                          # the replay: the same five calls, typed out
        want_top = random.randint(0, 37 - 8)
        want_left = random.randint(0, 20 - 8)
        bits = [random.random() < 0.5, random.random() < 0.5, random.random() < 0.5]
        assert random.getstate() == after, seed                         # exactly these draws, no more
        assert (top, left, code) == (want_top, want_left, bits[0] | bits[1] << 1 | bits[2] << 2), seed
        assert 0 <= top <= 29 and 0 <= left <= 12 and type(code) is int
        now = np.random.get_state()
        assert now[0] == np_before[0] and np.array_equal(now[1], np_before[1]) and now[2:] == np_before[2:]
        assert torch.equal(torch.get_rng_state(), torch_before)
        codes.add(code)
    assert codes == set(range(8))
    random.seed(0)
    assert D.sample_paired_draw(8, 8, 8)[:2] == (0, 0)                  # an image of exactly the patch: one legal crop


def test_check_paired_records_refuses_each_bad_field_by_name(D):
    table = np.asarray([[0, 0, 10, 12], [960, 360, 8, 8]], dtype=np.int64)
    ok = np.asarray([[0, 2, 4, 7], [1, 0, 0, 0], [0, 0, 0, 5]], dtype=np.int32)
    out = D.check_paired_records(ok, table, 8)
    assert out.dtype == np.int32 and out.shape == (3, 4) and np.array_equal(out, ok)
    for bad, word in (([2, 0, 0, 0], "image index 2"), ([-1, 0, 0, 0], "image index -1"), ([0, 3, 0, 0], "top 3"), ([0, -1, 0, 0], "top -1"),
                      ([0, 0, 5, 0], "left 5"), ([0, 0, -2, 0], "left -2"), ([1, 1, 0, 0], "top 1"), ([1, 0, 1, 0], "left 1"),
                      ([0, 0, 0, 8], "code 8"), ([0, 0, 0, -1], "code -1")):
        rec = ok.copy()
        rec[1] = bad
        with pytest.raises(ValueError, match=f"paired records: {word} of record 1"):
            D.check_paired_records(rec, table, 8)
    with pytest.raises(ValueError, match="paired records"):
        D.check_paired_records(np.zeros((2, 3), np.int32), table, 8)
    with pytest.raises(ValueError, match="paired records"):
        D.check_paired_records(np.zeros((1, 4), np.float32), table, 8)


def test_header_declares_the_entry_once_and_the_library_exports_it(D):
    import ctypes as C
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert len(re.findall(r"\bint resr_pair_batch\(", text)) == 1
    assert "resr_pair_batch" in _lib.exported_symbols()
    res, args = _lib._PROTOS["resr_pair_batch"]
    assert res is C.c_int and len(args) == 11
    assert callable(C.CDLL(_lib.LIB_PATH).resr_pair_batch)              # the built library itself, not the binding's table
    assert callable(_lib.lib().resr_pair_batch)


# ---- config ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def config(D, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(source=None, lr_dir=None):
        for name, value in (("RESR_DATA_SOURCE", source), ("RESR_PAIRED_LR_DIR", lr_dir)):
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


def test_config_takes_both_paired_sources_with_their_lr_directory(config, monkeypatch):
    for source in ("paired", "paired_loader"):
        c = config(source, "/data/pairs/lr")
        assert c.data_source == source and c.paired_lr_image_dir == "/data/pairs/lr" and source in c.PAIRED_DATA_SOURCES
        assert c.paired_patch() == c.image_size // c.upscale_factor == 64
        with pytest.raises(ValueError, match="RESR_PAIRED_LR_DIR"):
            config(source)
    c = config()                                                        # the default is untouched, and needs no LR directory
    assert c.data_source == "loader" and c.paired_lr_image_dir == ""
    assert config("device").data_source == "device"
    with pytest.raises(ValueError, match="RESR_DATA_SOURCE"):
        config("hbm", "/data/pairs/lr")
    c = config("paired", "/data/pairs/lr")
    monkeypatch.setattr(c, "image_size", 250)
    with pytest.raises(ValueError, match="image_size=250.*upscale_factor=4"):
        c.paired_patch()


# ---- what from_dirs refuses, a device never touched ----------------------------------------------------------------------------------
def _png(path, h, w, seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def _dirs(tmp_path, name, sizes, scale=4):
    """sizes: file name -> (lr_h, lr_w) or ((hr_h, hr_w), (lr_h, lr_w)); None on a side leaves that file out."""
    hr_dir, lr_dir = tmp_path / name / "hr", tmp_path / name / "lr"
    hr_dir.mkdir(parents=True)
    lr_dir.mkdir()
    for k, (fname, size) in enumerate(sizes.items()):
        hr_size, lr_size = size if isinstance(size[0], (tuple, type(None))) else ((scale * size[0], scale * size[1]), size)
        if hr_size is not None:
            _png(str(hr_dir / fname), *hr_size, seed=2 * k)
        if lr_size is not None:
            _png(str(lr_dir / fname), *lr_size, seed=2 * k + 1)
    return str(hr_dir), str(lr_dir)


def test_from_dirs_refuses_bad_sets_before_any_device_work(D, tmp_path):
    dev = torch.device("cuda", 0)      # never reached: every refusal below comes first
    good = {"a.png": (8, 9), "b.png": (12, 8)}
    hr_dir, lr_dir = _dirs(tmp_path, "no_lr", dict(good, **{"c.png": ((32, 32), None)}))
    with pytest.raises(ValueError, match=r"hr.c\.png has no partner .*lr.c\.png"):
        D.PairedDeviceSource.from_dirs(hr_dir, lr_dir, 1, 8, 4, dev)
    hr_dir, lr_dir = _dirs(tmp_path, "no_hr", dict(good, **{"c.png": (None, (8, 8))}))
    with pytest.raises(ValueError, match=r"lr.c\.png has no partner .*hr.c\.png"):
        D.PairedDeviceSource.from_dirs(hr_dir, lr_dir, 1, 8, 4, dev)
    hr_dir, lr_dir = _dirs(tmp_path, "ratio", dict(good, **{"c.png": ((32, 33), (8, 8))}))
    with pytest.raises(ValueError, match=r"c\.png: the HR side is 33x32, not 4 x the 8x8 LR side"):
        D.PairedDeviceSource.from_dirs(hr_dir, lr_dir, 1, 8, 4, dev)
    with pytest.raises(ValueError, match=r"not 2 x"):                   # a right set under the wrong scale
        D.PairedDeviceSource.from_dirs(*_dirs(tmp_path, "scale", good), 1, 8, 2, dev)
    hr_dir, lr_dir = _dirs(tmp_path, "small", dict(good, **{"c.png": (8, 7)}))
    with pytest.raises(ValueError, match=r"c\.png: the 7x8 LR side is below the patch 8"):
        D.PairedDeviceSource.from_dirs(hr_dir, lr_dir, 1, 8, 4, dev)
    hr_dir, lr_dir = _dirs(tmp_path, "budget", good)
    total = (8 * 9 + 12 * 8) * 3 * 17                                   # both arenas count
    with pytest.raises(ValueError, match=f"max_bytes={total - 1}"):
        D.PairedDeviceSource.from_dirs(hr_dir, lr_dir, 1, 8, 4, dev, max_bytes=total - 1)
    with pytest.raises(ValueError, match="no files"):
        D.PairedDeviceSource.from_dirs(*_dirs(tmp_path, "empty", {}), 1, 8, 4, dev)
    hr, lr = np.zeros((32, 32, 3), np.uint8), np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="max_bytes"):
        D.PairedDeviceSource.from_arrays([hr], [lr], 1, 8, 4, dev, max_bytes=32 * 32 * 3 + 8 * 8 * 3 - 1)
    for hr_list, lr_list, word in (([hr, hr], [lr], "2 HR images for 1"), ([hr[:31]], [lr], "pair 0"), ([hr], [lr[:7]], "pair 0"),
                                   ([hr.astype(np.float32)], [lr], "uint8")):
        with pytest.raises(ValueError, match=word):
            D.PairedDeviceSource.from_arrays(hr_list, lr_list, 1, 8, 4, dev)


# ---- the loader path ---------------------------------------------------------------------------------------------------------------
def test_paired_image_dataset_yields_the_definition_for_a_seeded_draw(D, tmp_path):
    from PIL import Image
    from real_esrgan_pytorch_amd.dataset import PairedImageDataset
    hr_dir, lr_dir = _dirs(tmp_path, "set", {"a.png": (9, 14), "b.png": (6, 6), "c.png": (17, 7)}, scale=3)
    data = PairedImageDataset(hr_dir, lr_dir, 6, 3)
    names = os.listdir(hr_dir)
    assert len(data) == 3 and [os.path.basename(p) for p in data.hr_file_names] == names == [os.path.basename(p) for p in data.lr_file_names]
    for i, name in enumerate(names):
        hr = np.asarray(Image.open(os.path.join(hr_dir, name)).convert("RGB"))
        lr = np.asarray(Image.open(os.path.join(lr_dir, name)).convert("RGB"))
        random.seed(40 + i)
        top, left, code = D.sample_paired_draw(lr.shape[0], lr.shape[1], 6)
        after = random.getstate()
        want_lr, want_hr = D.paired_sample_np(hr, lr, top, left, code, 6, 3)
        random.seed(40 + i)
        item = data[i]
        assert random.getstate() == after                               # the sample's five draws and nothing else
        assert set(item) == {"lr", "hr"} and item["lr"].dtype == item["hr"].dtype == torch.float32
        assert item["lr"].shape == (3, 6, 6) and item["hr"].shape == (3, 18, 18)
        assert torch.equal(item["lr"], torch.from_numpy(want_lr)) and torch.equal(item["hr"], torch.from_numpy(want_hr)), name
    with pytest.raises(ValueError, match="below the patch"):
        PairedImageDataset(hr_dir, lr_dir, 7, 3)[names.index("b.png")]
    with pytest.raises(ValueError, match="no partner"):
        PairedImageDataset(hr_dir, str(tmp_path / "set"), 6, 3)
