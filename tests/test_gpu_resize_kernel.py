"""-m gpu: `resize_tile` of csrc/image_resize.hip, alone through the C ABI (resr_image_resize, fp32 and uint8 output), against the
bit-exact restatement of its definition in tests/resize_ref.py (proven on the CPU by tests/test_resize_ref.py: libm's fmaf, the nine
goldens, and the wrong kernels bit equality must reject).

How a result is judged
  * fp32: the int32 views are equal element by element; where the reference is NaN the kernel's result is NaN (a payload is not part
    of the result).  No tolerance.
  * uint8: the bytes are equal.  No exclusion band around integers.
  * every output lies between sentinel guards and is pre-filled (tests/gpu_util.Out): the guards must survive and every element in
    range must have been written -- the row stores of the small tiles (heads, tails, rows shorter than a dword) are where that can go
    wrong.  The fp32 sentinel is a NaN no kernel produces; a uint8 output is launched twice, over two different fillings, and both
    results must be the reference's bytes, so no byte can pass by having been left alone.
  * every case that is about a tile asserts the tile resr_debug_resize_plan reports for its launch, fp32 and uint8: the eleven entries
    of choose_tile's list all run (tests/resize_ref.py TILE_OF; 1 x 2 is reached at r = 0.07), each on a 96 x 96 source and on a ragged
    97 x 131 one whose outputs are no multiple of the tile.
The cases are those of tests/resize_ref.py (`all_cases`): the tiles, r around and above 1, the smallest admitted sources, channel
groups and batches, per-axis and hand-made tables, tables without antialiasing, constant images on the uint8 clamps, non-finite pixels.
Every judgement goes to <diag_dir>/test_gpu_resize_kernel.json, per tile."""
import json
import os

import numpy as np
import pytest
import torch

from tests import resize_ref as rr
from tests.gpu_util import Out, dev

pytestmark = pytest.mark.gpu
CASES = rr.all_cases()
RECORDS = {}


@pytest.fixture(scope="module")
def L():
    import real_esrgan_pytorch_amd as pkg
    pkg._lib.lib()
    return pkg._lib


@pytest.fixture(scope="module", autouse=True)
def _write_diag(diag_dir):
    yield
    tiles = {}
    for rec in RECORDS.values():
        t = tiles.setdefault(rec["tile"], {"fp32_cases": 0, "fp32_bit_equal": 0, "u8_cases": 0, "u8_byte_equal": 0})
        t["fp32_cases"] += 1
        t["fp32_bit_equal"] += rec["fp32_equal"]
        if "u8_equal" in rec:
            t["u8_cases"] += 1
            t["u8_byte_equal"] += rec["u8_equal"]
    with open(os.path.join(diag_dir, "test_gpu_resize_kernel.json"), "w") as f:
        json.dump({"tiles": tiles, "cases": RECORDS}, f, indent=1, sort_keys=True)


def _launch(L, case, u8, fill=None):
    """resr_image_resize of the case into a guarded, sentinel-filled output; the result as the kernel left it.  fill: the byte a
    uint8 output holds before the launch in place of the sentinel, which is itself a byte the kernel may produce."""
    x, iy, wy, ix, wx = (dev(a) for a in (case.x,) + case.tables())
    count = case.n * case.oh * case.ow * (3 if u8 else case.c)
    out = Out(count, np.uint8 if u8 else np.float32)
    if fill is not None:
        out.load(np.full(count, fill, np.uint8))
    rc = L.lib().resr_image_resize(L.ptr(x), out.ptr, case.n, case.c, case.h, case.w, case.oh, case.ow, L.ptr(iy), L.ptr(wy), case.taps_y,
                                   L.ptr(ix), L.ptr(wx), case.taps_x, 1 if u8 else 0, L.stream_ptr(x))
    assert rc == 0, (rc, L.lib().resr_last_error())
    got = out.read(written=not u8)            # synchronises; guards intact, every fp32 element written
    return got.reshape((case.n, case.oh, case.ow, 3) if u8 else (case.n, case.c, case.oh, case.ow))


def _first(mask):
    return np.argwhere(mask)[:4].tolist()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_is_the_definition_bit_for_bit(L, case):
    lib = L.lib()
    plan = case.plan(lib, rr.F32)
    assert plan is not None, lib.resr_last_error()
    if case.tile is not None:
        assert (plan.th, plan.tw) == case.tile, (case.name, plan)
    rec = RECORDS[case.name] = {"tile": f"{plan.th}x{plan.tw}", "tiles_per_axis": list(case.tiles_per_axis(plan)), "fp32_equal": False}
    ref = case.ref_f32()
    got = _launch(L, case, u8=False)
    nan = np.isnan(ref)
    bits, want = got.view(np.int32), ref.view(np.int32)
    wrong = (np.isnan(got) != nan) | (~nan & (bits != want))
    print(f"{case.name}: tile {plan.th}x{plan.tw}, {case.tiles_per_axis(plan)} tiles, fp32 elements that differ in bits: "
          f"{int(wrong.sum())} of {ref.size} ({int(nan.sum())} NaN due)")
    assert not wrong.any(), (f"{case.name}: {int(wrong.sum())} of {ref.size} fp32 results are not the definition's bits, first at "
                             f"{_first(wrong)}: got {got[wrong][:4].tolist()}, want {ref[wrong][:4].tolist()}")
    rec["fp32_equal"] = True
    if case.name == "one_tap_identity":       # fmaf(v, 1, 0) twice: the output's bits are the input's
        assert np.array_equal(bits, case.x.view(np.int32))
    if case.name.startswith("nonfinite"):
        assert 0 < nan.sum() < ref.size and np.isinf(ref).any()
    if not case.u8:
        return
    # ---- the same launch with uint8 output: [N, oh, ow, 3] ----
    pu = case.plan(lib, rr.U8)
    assert pu is not None and (case.tile is None or (pu.th, pu.tw) == case.tile), (case.name, pu)
    rec["u8_equal"] = False
    rec["u8_tile"] = f"{pu.th}x{pu.tw}"
    ref8 = case.ref_u8()
    # two launches over different fillings: a byte the kernel never wrote differs from the reference in at least one of them
    got8, again = _launch(L, case, u8=True), _launch(L, case, u8=True, fill=0x5A)
    wrong = (got8 != ref8) | (again != ref8)
    print(f"{case.name}: uint8 tile {pu.th}x{pu.tw}, bytes that differ: {int(wrong.sum())} of {ref8.size}")
    assert not wrong.any(), (f"{case.name}: {int(wrong.sum())} of {ref8.size} bytes are not the definition's, first at {_first(wrong)}: "
                             f"got {got8[wrong][:4].tolist()}, want {ref8[wrong][:4].tolist()}")
    rec["u8_equal"] = True
    if case.name.startswith("nonfinite"):     # a NaN sum is byte 0
        assert (got8[np.isnan(ref).transpose(0, 2, 3, 1)] == 0).all()
    if case.name.startswith("constant"):      # the values sit on integers and on both clamps
        assert len(np.unique(ref8)) <= 3
