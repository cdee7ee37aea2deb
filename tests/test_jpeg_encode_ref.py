"""The numpy definition of the device JPEG encoder (tests/jpeg_encode_ref.py) held to itself, to float64 and to Pillow.  No GPU.

Measured on the three fidelity images (sample_38x30.png, a 64x48 gradient with noise, 33x47 uniform noise; qualities 10, 50, 75, 90, 95,
100; both subsamplings; Pillow 12.2 / libjpeg-turbo with the same quality, subsampling, optimize=False and restart_marker_blocks = our
interval): the largest PSNR deficit of Pillow's decode of our file against Pillow's decode of its own is 0.0452 dB (scattered: ours is
level or ahead in 22 of the 36 cases, by up to 0.29 dB at quality 100), the largest size excess 82 bytes.  The gates are twice those.  Every size
excess is at 4:2:0 on the two images whose sides are no multiple of 16: libjpeg codes the blocks of an MCU that lie wholly outside the
image as empty "dummy" blocks, this encoder codes the replicated edge; on the 64x48 image ours is the smaller file in all twelve cases."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_encode_cases as K
from tests import jpeg_encode_ref as J

PSNR_GATE_DB = 2 * 0.0452
SIZE_GATE_BYTES = 2 * 82
FIDELITY_QUALITIES = (10, 50, 75, 90, 95, 100)
PILLOW_SUBSAMPLING = {"444": 0, "420": 2}


def _fidelity_images():
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:48, 0:64]
    gradient = np.clip(np.stack([x * 4, y * 5, (x + y) * 2], -1) + rng.integers(-8, 9, (48, 64, 3)), 0, 255).astype(np.uint8)
    return {"sample_38x30": np.asarray(Image.open(K.GOLDEN_PNG).convert("RGB")), "gradient_64x48": gradient,
            "noise_33x47": rng.integers(0, 256, (47, 33, 3), dtype=np.uint8)}


def _open(data: bytes) -> Image.Image:
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(data))
        image.load()
    return image


def _pillow_file(image, quality, subsampling, interval) -> bytes:
    out = io.BytesIO()
    Image.fromarray(image).save(out, "JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[subsampling], optimize=False, restart_marker_blocks=interval)
    return out.getvalue()


def _psnr(a, b) -> float:
    return float(10 * np.log10(65025.0 / np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


@pytest.mark.parametrize("name", list(K.CASES))
def test_round_trip_and_pillow_reads_the_file(name):
    image, quality, subsampling, interval = K.CASES[name]
    data = K.reference(name)
    want = J.frontend_np(image, quality, subsampling)
    assert np.array_equal(J.decode_scan_np(data), want)
    opened = _open(data)          # no warning, the whole scan decoded
    assert opened.size == (image.shape[1], image.shape[0]) and opened.mode == "RGB" and opened.format == "JPEG"
    info = J.parse_np(data)
    assert info["interval"] == (J.DEFAULT_RESTART_INTERVAL if interval is None else interval)


def test_the_contents_are_what_their_names_say():
    z = J.frontend_np(*K.CASES["isolated-444"][:3])[:, 0]          # the luma blocks
    for block, position in zip(z, K.ISOLATED):
        assert block[0] == 0 and list(np.flatnonzero(block)) == [position], (position, np.flatnonzero(block))
    assert not J.frontend_np(*K.CASES["isolated-444"][:3])[:, 1:].any()
    assert not J.frontend_np(*K.CASES["flat-420"][:3])[..., 1:].any()
    dc = J.frontend_np(*K.CASES["checker-444"][:3])[:, 0, 0]
    assert set(dc) == {-1024, 1016} and np.abs(np.diff(dc)).max() == 2040          # size 11, the largest there is
    data = K.reference("noise-q100-444")
    scan = J.parse_np(data)["scan"]
    assert scan.count(b"\xff\x00") >= 10                                           # stuffing is exercised
    assert J.frontend_np(*K.CASES["noise-q100-444"][:3])[..., 63].any()                # blocks that end without an EOB
    # the segment counts the names promise
    for name, segments in (("one-whole-segment-420", 1), ("one-short-segment-444", 1), ("interval1-444", 15), ("interval5-444", 4), ("shape-24x200-444", 10),
                           ("several-workgroups-420", 115)):
        scan = J.parse_np(K.reference(name))["scan"]
        markers = sum(1 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7)
        assert markers == segments - 1, (name, markers)


def test_grey_is_exact_and_no_clamp_is_needed():
    v = np.arange(256, dtype=np.uint8)
    for sub in J.SUBSAMPLINGS:
        s = J.samples_np(np.repeat(np.repeat(v.reshape(16, 16, 1), 3, axis=2), 16, axis=0).repeat(16, axis=1), sub)      # 16x16 patches of (v, v, v)
        nb = s.shape[2]
        assert np.array_equal(np.unique(s[:, :, :nb - 2] + 128), np.arange(256)) and not s[:, :, nb - 2:].any()          # Y = v, Cb = Cr = 128
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8).reshape(8, 1, 3)
    for sub in J.SUBSAMPLINGS:
        s = J.samples_np(np.repeat(np.repeat(corners, 16, axis=0), 16, axis=1), sub) + 128
        assert s.min() == 0 and s.max() == 255          # the extremes are reached and not passed


@pytest.mark.parametrize("quality", [1, 10, 25, 49, 50, 51, 75, 90, 95, 100])
def test_quantiser_tables_are_pillows(quality):
    image = K.gradient(16, 16)
    ours = _open(J.encode_jpeg_np(image, quality, "420")).quantization
    theirs = _open(_pillow_file(image, quality, "420", 0)).quantization
    assert {k: list(v) for k, v in ours.items()} == {k: list(v) for k, v in theirs.items()}


def test_huffman_tables_are_the_ones_pillow_writes():
    image = K.gradient(16, 16)
    assert J.parse_np(J.encode_jpeg_np(image, 75, "444"))["tables"] == J.parse_np(_pillow_file(image, 75, "444", 0))["tables"]


def test_fidelity_and_size_against_pillow(capsys):
    worst_db, worst_bytes, ahead, lines = 0.0, 0, 0, []
    for name, image in _fidelity_images().items():
        for sub in J.SUBSAMPLINGS:
            for quality in FIDELITY_QUALITIES:
                ours = J.encode_jpeg_np(image, quality, sub)
                theirs = _pillow_file(image, quality, sub, J.DEFAULT_RESTART_INTERVAL)
                p_ours, p_theirs = _psnr(_open(ours), image), _psnr(_open(theirs), image)
                plain = len(J.encode_jpeg_np(image, quality, sub, 0))
                lines.append(f"{name} {sub} q{quality}: PSNR ours {p_ours:.3f} Pillow {p_theirs:.3f} dB; bytes ours {len(ours)} Pillow {len(theirs)}; "
                             f"restart markers cost {len(ours) - plain} bytes over interval 0 ({plain})")
                worst_db, worst_bytes = max(worst_db, p_theirs - p_ours), max(worst_bytes, len(ours) - len(theirs))
                ahead += p_ours >= p_theirs
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\nlargest PSNR deficit {worst_db:.4f} dB, largest size excess {worst_bytes} bytes, ours ahead in {ahead} of {len(lines)}")
    assert worst_db <= PSNR_GATE_DB, worst_db
    assert worst_bytes <= SIZE_GATE_BYTES, worst_bytes


def test_coefficients_against_float64():
    """G / 2^13 against a float64 DCT of the same samples.  Every entry of the Q20 matrix is off by at most e = 2^-21 of its real value,
    so F / 2^40 = sum (c + e1)(c' + e2) s is off by at most 128 (2 * 8 e A + 64 e^2) with A = 2.8285 the largest absolute row sum of the
    real matrix (row 0: 8 / (2 sqrt 2)); the rounding to Q13 adds 2^-14.  A quantised coefficient can then differ from
    round(float64 / step) only where the float64 value lies within bound / step of a tie."""
    e, a = 2.0 ** -21, 8 / (2 * np.sqrt(2.0))
    bound = 128 * (2 * 8 * e * a + 64 * e * e) + 2.0 ** -14
    assert bound < 2.9e-3
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    c = 0.5 * np.where(u == 0, 1 / np.sqrt(2.0), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16)
    assert np.abs(c).sum(axis=1).max() <= a + 1e-12
    differing = explained = total = 0
    for name in ("noise-q100-444", "noise-q50-420", "shape-33x47-444", "checker-444", "photo-420", "noise-q1-444"):
        image, quality, sub, _ = K.CASES[name]
        s = J.samples_np(image, sub)
        g = J.dct_q13_np(s)
        f = np.einsum("uy,...yx,vx->...uv", c, s.astype(np.float64), c)
        assert np.abs(g / 8192.0 - f).max() <= bound, name
        q = J.quant_tables(quality)
        nb = s.shape[2]
        steps = np.stack([q[0]] * (nb - 2) + [q[1], q[1]]).reshape(nb, 8, 8).astype(np.float64)
        ours = J.quantise_np(g.reshape(g.shape[:3] + (64,)), steps.reshape(nb, 64).astype(np.int64)).reshape(g.shape)
        ratio = f / steps
        theirs = np.sign(ratio) * np.floor(np.abs(ratio) + 0.5)
        differ = ours != theirs
        near_tie = np.abs(np.abs(ratio) - np.floor(np.abs(ratio)) - 0.5) <= bound / steps + 1e-12
        differing += int(differ.sum())
        explained += int((differ & near_tie).sum())
        total += differ.size
        assert not (differ & ~near_tie).any(), name
        assert np.abs(ours - theirs).max() <= 1
    assert differing == explained and differing < total / 200          # the bound explains every one, and they are rare


def test_refusals_of_the_definition():
    image = K.noise(8, 8)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            J.encode_jpeg_np(image, bad, "420")
    with pytest.raises(ValueError, match="subsampling"):
        J.encode_jpeg_np(image, 75, "422")
    with pytest.raises(ValueError, match="restart_interval"):
        J.encode_jpeg_np(image, 75, "420", 65536)
    with pytest.raises(ValueError, match="uint8"):
        J.encode_jpeg_np(image.astype(np.int32), 75, "420")
