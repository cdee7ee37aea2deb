"""CPU: the surface of outscale for the image modes (grey, RGBA and 16-bit images through a resizing tail) -- the three C-ABI names
(exported, declared once, bound), every refusal of resr_compact_forward_image_scaled before any launch, the fits query and the
debug plan against a restatement of the kernel's LDS budget, the Python signatures and the CLI switch.  Nothing here touches a
device: a call that got as far as a launch would not return RESR_ERR_ARG."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

from tests.test_image_modes_surface import ERR_ARG, ERR_WORKSPACE, LOAD_ALIGN, MODES, _desc, _fake
from tests.test_resize_surface import LDS_BUDGET, PLAN_MIXED, PLAN_SCALES, TILE_LIST, _span_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, FITS, DEBUG = "resr_compact_forward_image_scaled", "resr_compact_image_scaled_fits", "resr_debug_image_resize_plan"
PLAN_LENGTHS = (1, 2, 3, 5, 8, 13, 24, 25, 33, 37, 64, 96, 139, 270, 480)        # LR lengths; the HR frame is s times as long


@pytest.fixture(scope="module")
def R():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R


def test_symbols_exported_declared_once_and_bound(R):
    lib = C.CDLL(R._lib.LIB_PATH)
    text = {h: re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("resr.h", "resr_debug.h")}
    for name, header in ((ENTRY, "resr.h"), (FITS, "resr.h"), (DEBUG, "resr_debug.h")):
        assert hasattr(lib, name), name
        counts = {h: len(re.findall(r"\b%s\s*\(" % name, code)) for h, code in text.items()}
        assert counts == {h: int(h == header) for h in text}, (name, counts)
        assert name in R._lib.exported_symbols(), name
    assert R._lib.lib().resr_version() == R._lib.RESR_VERSION == 3            # nothing an existing caller reads has moved
    assert [f[0] for f in R._lib.ImageDesc._fields_] == ["channels", "bits"] and C.sizeof(R._lib.ImageDesc) == 8
    # each of the new host functions is declared once, in the internal header
    host = open(os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "host_api.h")).read()
    for name in ("compact_tail_image_scaled", "image_scaled_plan"):
        assert len(re.findall(r"\b%s\(" % name, host)) == 1, name
    # image_pixel and grey_of keep one definition, in the header both kernel files include
    csrc = os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc")
    for name in ("image_pixel", "grey_of"):
        defs = {f: len(re.findall(r"__forceinline__ \w+ %s\(" % name, open(os.path.join(csrc, f)).read()))
                for f in os.listdir(csrc) if f.endswith((".h", ".hip"))}
        assert {f: n for f, n in defs.items() if n} == {"yuv.h": 1}, (name, defs)


def test_python_signatures_and_formats(R):
    for fn in (R.upscale_image, R.SRVGGNetCompact.forward_image):
        params = inspect.signature(fn).parameters
        for name in ("outscale", "plan"):
            assert name in params and params[name].default is None, (fn, name)
    assert list(inspect.signature(R.upscale_image).parameters)[:3] == ["model", "images", "halo"]
    assert tuple(R.PIXEL_FORMATS) == R.FrameStream.PIX_FMTS == ("rgb24", "i420", "nv12", "i420p10", "p010")
    assert not hasattr(R.Generator, "forward_image") and not hasattr(R.Generator, "forward_u8")


def test_keep_mode_with_outscale_parses(R):
    from real_esrgan_pytorch_amd import inference_frames
    p = inference_frames.get_parser()
    a = p.parse_args(["--inputs_dir", "D", "--output_dir", "O", "--weights_path", "W", "--keep_mode", "--outscale", "2"])
    assert a.keep_mode is True and a.outscale == 2.0
    assert "outscale" in inspect.signature(inference_frames.upscale_kept).parameters


# ---- the refusals of the C entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,bits", MODES)
def test_forward_image_scaled_refusals_need_no_gpu(R, channels, bits):
    L = R._lib
    lib = L.lib()
    keep, base = _fake()
    p = C.c_void_p(base)
    planes = 2 if channels == 4 else 1
    good, img = _desc(L, n=planes), L.ImageDesc(channels, bits)          # one 8 x 8 image through an x4 model, resized to 16 x 16
    ws = lib.resr_compact_workspace_bytes(C.byref(good))
    assert ws > 0

    def call(d=good, x=p, params=p, packed=p, workspace=p, nbytes=ws, y=p, oh=16, ow=16, idx_y=p, w_y=p, taps_y=10, idx_x=p, w_x=p,
             taps_x=10, im=img):
        return getattr(lib, ENTRY)(C.byref(d) if d is not None else None, x, params, packed, workspace, nbytes, y, oh, ow, idx_y, w_y,
                                   taps_y, idx_x, w_x, taps_x, C.byref(im) if im is not None else None, None)

    # everything passes up to the workspace, the last check before the first launch: the calls below stop earlier
    assert call(nbytes=0) == ERR_WORKSPACE
    for hole in ("x", "params", "packed", "workspace", "y", "im", "idx_y", "w_y", "idx_x", "w_x"):
        assert call(**{hole: None}, nbytes=0) == ERR_ARG, hole
        assert b"null" in lib.resr_last_error(), hole
    assert call(d=None, nbytes=0) == ERR_ARG
    for bad in (_desc(L, n=0), _desc(L, n=planes, h=0), L.CompactDesc(planes, 8, 8, 2, 5, 0, L.RESR_F16, 0), _desc(L, 2, 4096, 4096, L.RESR_F16X2)):
        assert call(d=bad, nbytes=0) == ERR_ARG
        assert b"descriptor" in lib.resr_last_error()
    for c in (0, 2, 5, -1):
        assert call(im=L.ImageDesc(c, bits), nbytes=0) == ERR_ARG
        assert b"channels" in lib.resr_last_error()
    for b in (0, 10, 12, 32):
        assert call(im=L.ImageDesc(channels, b), nbytes=0) == ERR_ARG
        assert b"bits" in lib.resr_last_error()
    odd = call(d=_desc(L, n=3), nbytes=0)                                # RGBA: N colour and N alpha images
    if channels == 4:
        assert odd == ERR_ARG and b"odd" in lib.resr_last_error()
    else:
        assert odd == ERR_WORKSPACE
    # y: 4 bytes in every mode (rows leave as dword stores), not the unscaled tail's 8 or 16
    assert call(y=C.c_void_p(base + 2), nbytes=0) == ERR_ARG
    assert b"4-byte aligned" in lib.resr_last_error()
    assert call(y=C.c_void_p(base + 4), nbytes=0) == ERR_WORKSPACE
    # x: the head's rule (an RGBA pixel is one load)
    la = LOAD_ALIGN[channels, bits]
    if la > 1:
        assert call(x=C.c_void_p(base + la // 2), nbytes=0) == ERR_ARG
        assert b"source images must be %d-byte aligned" % la in lib.resr_last_error()
    assert call(x=C.c_void_p(base + la), nbytes=0) == ERR_WORKSPACE
    # what the scaled uint8 entry refuses
    for kw in (dict(oh=0), dict(ow=0), dict(oh=-4), dict(ow=-1), dict(taps_y=0), dict(taps_x=0), dict(taps_y=4097), dict(taps_x=4097)):
        assert call(**kw, nbytes=0) == ERR_ARG, kw
    assert call(d=_desc(L, n=planes * 65536, h=1, w=1), nbytes=0) == ERR_ARG
    assert b"beyond the grid" in lib.resr_last_error()
    assert call(d=_desc(L, n=planes * 65535, h=1, w=1), nbytes=0) == ERR_WORKSPACE
    # a scale with no tile: the 200 x 200 taps of one output pixel are 3 * 200 * 201 floats of source alone
    assert call(d=_desc(L, n=planes, h=250, w=250), oh=20, ow=20, taps_y=200, taps_x=200, nbytes=0) == ERR_ARG
    assert b"does not fit" in lib.resr_last_error()
    assert getattr(lib, FITS)(250, 250, 4, 20, 20, 200, 200, channels, bits) == 0
    # the plan is the inference one: the same workspace, and too little of it is the float entry's code
    assert call(nbytes=ws - 1) == ERR_WORKSPACE
    assert lib.resr_compact_workspace_bytes(C.byref(good)) == ws
    del keep


# ---- the fits query and the debug plan -------------------------------------------------------------------------------------------------
def _expected_plan(h, w, oh, ow, py, px, channels, bits):
    """choose_tile and lds_bytes of csrc/image_resize.hip restated for an image output: the first tile of the list (odd ones too) whose
    tables, region, intermediate and staging buffer -- th * tw * C words of bits / 8 bytes, rounded up to 4 -- fit the budget."""
    for th, tw in TILE_LIST:
        rh, rw = _span_bound(min(th, oh), h, oh, py), _span_bound(min(tw, ow), w, ow, px)
        pitch = rw | 1
        lds = 4 * (2 * (th * py + tw * px) + 3 * (rh + th) * pitch) + (th * tw * channels * (bits // 8) + 3) // 4 * 4
        if lds <= LDS_BUDGET:
            return (th, tw, rh, rw, pitch, lds)
    return None


def test_fits_query_and_debug_plan_agree_with_the_lds_budget(R):
    from real_esrgan_pytorch_amd import imgproc
    lib = R._lib.lib()
    fits, debug = getattr(lib, FITS), getattr(lib, DEBUG)
    out6 = (C.c_int32 * 6)()
    tally = {"plans": 0, "refused": 0}

    def taps(n, r):
        try:
            return imgproc.resize_band_tables(n, math.ceil(n * r), r, True)[0].shape[1]
        except ValueError:
            return None                                                # a length the reflection rule refuses: no launch exists

    pairs = [(r, r) for r in PLAN_SCALES] + list(PLAN_MIXED)
    for s in (1, 2, 3, 4):
        for ry, rx in pairs:
            for i, h in enumerate(PLAN_LENGTHS):
                w = PLAN_LENGTHS[(5 * i + 2) % len(PLAN_LENGTHS)]
                py, px = taps(h * s, ry), taps(w * s, rx)
                if py is None or px is None:
                    continue
                oh, ow = math.ceil(h * s * ry), math.ceil(w * s * rx)
                for channels, bits in MODES:
                    want = _expected_plan(h * s, w * s, oh, ow, py, px, channels, bits)
                    what = (s, ry, rx, h, w, channels, bits)
                    for k in range(6):
                        out6[k] = -7
                    rc = debug(h, w, s, oh, ow, py, px, channels, bits, out6)
                    assert fits(h, w, s, oh, ow, py, px, channels, bits) == (want is not None), what
                    if want is None:
                        assert rc == ERR_ARG and list(out6) == [-7] * 6, what      # a refused plan leaves its output untouched
                        tally["refused"] += 1
                        continue
                    assert rc == 0 and tuple(out6) == want, (what, tuple(out6), want)
                    assert want[5] <= LDS_BUDGET
                    tally["plans"] += 1
                    tally[want[:2]] = tally.get(want[:2], 0) + 1
                    if (channels, bits) == (3, 8):                     # 8-bit RGB is the uint8 tail: its plan
                        u8 = (C.c_int32 * 6)()
                        assert lib.resr_debug_resize_plan(1, 3, h * s, w * s, oh, ow, py, px, 1, u8) == 0 and tuple(u8) == want, what
    print(f"image resize plans checked: {tally['plans']}, {tally['refused']} refused; per tile: { {k: v for k, v in tally.items() if isinstance(k, tuple)} }")
    assert tally["plans"] >= 5000 and tally["refused"] > 0
    assert all(tally.get(t, 0) > 0 for t in TILE_LIST), [t for t in TILE_LIST if not tally.get(t)]
    # the staging buffer is the mode's: C words of bits / 8 bytes per pixel of the tile
    sizes = {}
    for channels, bits in MODES:
        assert debug(270, 480, 4, 540, 960, 10, 10, channels, bits, out6) == 0 and list(out6)[:5] == [16, 32, 42, 74, 75]
        sizes[channels, bits] = out6[5]
    floats = 4 * (2 * (16 * 10 + 32 * 10) + 3 * (42 + 16) * 75)
    assert sizes == {(c, b): floats + 16 * 32 * c * b // 8 for c, b in MODES}
    # bad arguments: 0 from the query, RESR_ERR_ARG from the plan, nothing written
    good = dict(h=24, w=24, s=4, oh=48, ow=48, ty=10, tx=10, c=4, b=8)
    for kw in (dict(h=0), dict(w=-1), dict(s=0), dict(s=5), dict(oh=0), dict(ow=-2), dict(ty=0), dict(tx=4097), dict(c=2), dict(c=0), dict(b=10),
               dict(b=0), dict(h=1 << 30)):
        a = dict(good, **kw)
        args = (a["h"], a["w"], a["s"], a["oh"], a["ow"], a["ty"], a["tx"], a["c"], a["b"])
        for k in range(6):
            out6[k] = -7
        assert fits(*args) == 0 and debug(*args, out6) == ERR_ARG and list(out6) == [-7] * 6, kw
    assert debug(*(good[k] for k in ("h", "w", "s", "oh", "ow", "ty", "tx", "c", "b")), None) == ERR_ARG
    # the generic entry keeps refusing the image kinds: they have their own
    assert lib.resr_debug_resize_plan(1, 3, 96, 96, 48, 48, 10, 10, 4, out6) == ERR_ARG
