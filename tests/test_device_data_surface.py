"""CPU: the host definitions of the device-resident data source (device_data.py) against the loader path's own functions, the
declarations of its two entries, `config.data_source`, and what the source refuses before it touches a device."""
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


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _states_equal(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def test_blur_params_reproduce_sample_blur_kernels_and_both_generators(D):
    from real_esrgan_pytorch_amd.degrade import sample_blur_kernels
    families = set()
    for seed in range(200):
        _seed(seed)
        want = sample_blur_kernels()
        after_want = (random.getstate(), np.random.get_state())
        _seed(seed)
        rec = D.sample_blur_params()
        after_got = (random.getstate(), np.random.get_state())
        assert rec.shape == (3, D.RECORD) and rec.dtype == np.float64
        got = D.blur_kernels_from_params_np(rec)
        assert got.shape == (3, 21, 21) and got.dtype == np.float32
        for k in range(3):
            assert want[k].dtype == np.float32 and np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (seed, k)
        assert _states_equal(after_want, after_got), seed
        families |= {(int(r[0]), bool(r[6])) for r in rec}
    # 200 seeds reach every family, isotropic and anisotropic
    assert families == {(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, False), (4, False)}, families


@pytest.mark.parametrize("side", [5, 6, 24, 33])
def test_augment_np_is_the_imgproc_chain(D, side):
    from real_esrgan_pytorch_amd import imgproc
    tile = np.random.default_rng(side).integers(0, 256, (side, side, 3), dtype=np.uint8)
    image = tile.astype(np.float32) / 255.0
    codes = set()
    for seed in range(64):
        random.seed(seed)
        want = imgproc.random_rotate(image, [0, 90, 180, 270])
        want = imgproc.random_horizontally_flip(want, 0.5)
        want = imgproc.random_vertically_flip(want, 0.5)
        want = imgproc.image_to_tensor(want, False, False)
        after = random.getstate()
        random.seed(seed)
        code = D.sample_augment()
        assert random.getstate() == after and 0 <= code < 16
        got = D.augment_np(tile, code)
        assert got.dtype == torch.float32 and got.shape == (3, side, side) and torch.equal(got, want), (seed, code)
        codes.add(code)
    assert codes == set(range(16))


def test_augment_np_keeps_the_zero_line_of_an_even_side(D):
    tile = np.full((6, 6, 3), 255, dtype=np.uint8)
    assert float(D.augment_np(tile, 0).min()) == 1.0
    row0, col0 = (slice(None), 0, slice(None)), (slice(None), slice(None), 0)
    for code, zeros, kept in ((1, [row0], 30), (2, [row0, col0], 25), (3, [col0], 30)):      # 180 loses a row AND a column
        out = D.augment_np(tile, code)
        assert float(out.sum()) == 3 * kept and all(float(out[z].abs().max()) == 0.0 for z in zeros), code
    assert float(D.augment_np(np.full((5, 5, 3), 255, dtype=np.uint8), 2).min()) == 1.0      # odd sides lose nothing


def test_header_declares_both_entries(D):
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert re.search(r"\bint resr_tile_batch\(", text) and re.search(r"\bint resr_blur_kernels\(", text)
    assert {"resr_tile_batch", "resr_blur_kernels"} <= set(_lib.exported_symbols())
    assert len(_lib._PROTOS["resr_tile_batch"][1]) == 8 and len(_lib._PROTOS["resr_blur_kernels"][1]) == 5
    assert _lib.RESR_BLUR_RECORD == D.RECORD and _lib.RESR_BLUR_MAX_SIDE >= 21
    assert [getattr(_lib, "RESR_BLUR_" + f.upper()) for f in D.FAMILIES] == [0, 1, 2, 3, 4]
    assert callable(_lib.lib().resr_tile_batch) and callable(_lib.lib().resr_blur_kernels)


def test_blur_records_outside_the_definition_are_refused(D):
    ok = [0, 7, 1.0, 1.0, 0.0, 1.0, 0, 0.0]
    D.check_blur_records([ok])
    for bad in ([5, 7, 1, 1, 0, 1, 0, 0], [-1, 7, 1, 1, 0, 1, 0, 0], [0, 8, 1, 1, 0, 1, 0, 0], [0, 23, 1, 1, 0, 1, 0, 0],
                [3, 0, 0, 0, 0, 1, 0, 1.0], [4, 3, 0, 0, 0, 1, 0, 0], [0, 7, 0.0, 1, 0, 1, 0, 0], [0, 7.5, 1, 1, 0, 1, 0, 0],
                [0, 7, float("nan"), 1, 0, 1, 0, 0]):
        with pytest.raises(ValueError, match="blur kernels"):
            D.check_blur_records([bad])
    with pytest.raises(ValueError, match="odd"):
        D.check_blur_records([ok], K=20)


@pytest.fixture
def config(D, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(value=None):
        monkeypatch.delenv("RESR_DATA_SOURCE", raising=False)
        if value is not None:
            monkeypatch.setenv("RESR_DATA_SOURCE", value)
        return importlib.reload(module)
    yield reload
    monkeypatch.undo()
    importlib.reload(module)
    torch.set_rng_state(state[0])
    random.setstate(state[1])
    np.random.set_state(state[2])


def test_data_source_defaults_to_the_loader_and_refuses_other_names(config):
    assert config().data_source == "loader"
    assert config("device").data_source == "device"
    assert config("loader").data_source == "loader"
    with pytest.raises(ValueError, match="RESR_DATA_SOURCE"):
        config("hbm")


def _png(path, h, w, seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def test_source_refuses_bad_tiles_and_budgets_before_any_device_work(D, tmp_path):
    dev = torch.device("cuda", 0)      # never reached: every refusal below comes first
    d1 = tmp_path / "wide"
    d1.mkdir()
    _png(str(d1 / "a.png"), 24, 32)
    with pytest.raises(ValueError, match=r"a\.png.*square"):
        D.DeviceTileSource.from_dir(str(d1), 1, dev)
    d2 = tmp_path / "mixed"
    d2.mkdir()
    for i in range(3):
        _png(str(d2 / f"{i}.png"), 24, 24, i)
    _png(str(d2 / "odd_one.png"), 16, 16)
    first = os.listdir(str(d2))[0]      # the first file sets the size; the message names the first file that differs from it
    differs = "odd_one.png" if first != "odd_one.png" else next(n for n in os.listdir(str(d2)) if n != first)
    with pytest.raises(ValueError, match=re.escape(differs) + r" is \d+x\d+, expected"):
        D.DeviceTileSource.from_dir(str(d2), 1, dev)
    d3 = tmp_path / "four"
    d3.mkdir()
    for i in range(4):
        _png(str(d3 / f"{i}.png"), 24, 24, i)
    with pytest.raises(ValueError, match="max_bytes"):
        D.DeviceTileSource.from_dir(str(d3), 1, dev, max_bytes=4 * 24 * 24 * 3 - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        D.DeviceTileSource.from_array(np.zeros((4, 8, 8, 3), np.uint8), 1, dev, max_bytes=4 * 8 * 8 * 3 - 1)
    for bad in (np.zeros((4, 8, 6, 3), np.uint8), np.zeros((4, 8, 8, 3), np.float32), np.zeros((4, 8, 8, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8 .M,T,T,3."):
            D.DeviceTileSource.from_array(bad, 1, dev)
