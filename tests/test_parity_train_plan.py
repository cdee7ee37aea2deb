"""CPU: the output-parity training plan (x2_plan bit 11, RESR_X2_PLAN_MX_TRAIN_FORWARD = 2048) is accepted by the module with its four
prerequisites -- the inference MX forward (1 + 32 + 64) and the f16 backward pass (256) -- and refused without any one of them."""
import pytest


def test_output_parity_plan_constructs():
    import real_esrgan_pytorch_amd as R
    L = R._lib
    assert L.X2_PLAN_MX_TRAIN_FORWARD == 2048
    assert L.X2_PLAN_OUTPUT_PARITY == 1 + 32 + 64 + 256 + 2048 == 2401
    assert L.CONV_MX_SIGNBITS == 1 << 13
    g = R.Generator(3, 3, 4, precision="exact16", x2_plan=2401)
    assert g.x2_plan == 2401
    # the MX backward bits on top stay legal (bit 8 overrides them in the backward pass)
    R.Generator(3, 3, 4, precision="exact16", x2_plan=2401 | 2 | 8 | 16 | 128 | 512)


@pytest.mark.parametrize("missing", [1, 32, 64, 256])
def test_output_parity_bit_needs_its_prerequisites(missing):
    import real_esrgan_pytorch_amd as R
    with pytest.raises(ValueError):
        R.Generator(3, 3, 4, precision="exact16", x2_plan=2401 & ~missing)


def test_x2_plan_range():
    import real_esrgan_pytorch_amd as R
    with pytest.raises(ValueError):
        R.Generator(3, 3, 4, precision="exact16", x2_plan=4096)
