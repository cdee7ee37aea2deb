"""CPU: the prerequisite rules of ResrGeneratorDesc.x2_plan live once, in csrc/generator.hip resolve_x2_plan; the module asks the library
(_lib.x2_plan_error: a size query on a minimal descriptor).  Its answer and every entry point that takes the descriptor must refuse
exactly the same plans, over all 4096 of them and both `training` values, and name the broken rule's bit."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R._lib


def _desc(L, dtype, training, plan):
    return L.GeneratorDesc(1, 24, 24, 3, 3, 4, 2, dtype, training, 0, plan, 0)


# one refused plan per rule: (plan, the bit whose rule it breaks)
REFUSED = [(4, 4), (16, 16), (32, 32), (64 | 1, 64), (128 | 512, 512), (1024 | 128 | 8, 1024), (2048 | 1 | 32 | 64, 2048),
           (128 | 4 | 2, 128), (4096, 4096)]


def test_module_and_library_refuse_the_same_plans(L):
    lib = L.lib()
    refused = 0
    for plan in range(4096):
        ok = L.x2_plan_error(plan) is None
        refused += not ok
        for training in (0, 1):
            d = _desc(L, L.RESR_F16X2, training, plan)
            assert (lib.resr_generator_workspace_bytes(C.byref(d)) > 0) == ok, (plan, training)
            assert (lib.resr_generator_pack_table(C.byref(d), training, None, 0) > 0) == ok, (plan, training)
    assert 0 < refused < 4096
    for plan in (4096, 1 << 20):
        assert L.x2_plan_error(plan) is not None
        for training in (0, 1):
            d = _desc(L, L.RESR_F16X2, training, plan)
            assert lib.resr_generator_workspace_bytes(C.byref(d)) == 0
            assert lib.resr_generator_pack_table(C.byref(d), training, None, 0) < 0


def test_every_entry_point_refuses_and_names_the_rule(L):
    lib = L.lib()
    for plan, bit in REFUSED:
        assert L.x2_plan_error(plan) is not None and str(bit) in L.x2_plan_error(plan), plan
        for training in (0, 1):
            d = _desc(L, L.RESR_F16X2, training, plan)
            for size in (lib.resr_generator_workspace_bytes, lib.resr_generator_param_count, lib.resr_generator_mx_offset,
                         lib.resr_generator_chain_state_bytes):
                assert size(C.byref(d)) == 0, (plan, size.__name__)
            assert lib.resr_generator_packed_bytes(C.byref(d), training) == 0
            assert lib.resr_generator_workspace_bytes(C.byref(d)) == 0
            assert str(bit) in lib.resr_last_error().decode(), (plan, lib.resr_last_error())
            # (the descriptor is refused before any pointer is looked at: these calls reach no GPU)
            assert lib.resr_generator_pack_table(C.byref(d), 1, None, 0) == -1
            assert lib.resr_generator_buffer_offsets(C.byref(d), None, 0) == -1
            assert lib.resr_generator_forward(C.byref(d), None, None, None, None, 0, None, None) == -1
            assert str(bit) in lib.resr_last_error().decode()
            assert lib.resr_generator_backward(C.byref(d), None, None, None, None, 0, None, None, None, None, 0) == -1
            assert str(bit) in lib.resr_last_error().decode()


def test_other_dtypes_ignore_the_field(L):
    lib = L.lib()
    for dtype in (L.RESR_F16, L.RESR_F32):
        for training in (0, 1):
            d0 = _desc(L, dtype, training, 0)
            want = (lib.resr_generator_workspace_bytes(C.byref(d0)), lib.resr_generator_packed_bytes(C.byref(d0), 0),
                    lib.resr_generator_packed_bytes(C.byref(d0), 1))
            assert min(want) > 0
            for plan in [p for p, _ in REFUSED] + [1 << 20]:
                d = _desc(L, dtype, training, plan)
                got = (lib.resr_generator_workspace_bytes(C.byref(d)), lib.resr_generator_packed_bytes(C.byref(d), 0),
                       lib.resr_generator_packed_bytes(C.byref(d), 1))
                assert got == want, (dtype, training, plan)


def test_generator_raises_the_rules_text(L):
    import real_esrgan_pytorch_amd as R
    for plan, bit in REFUSED:
        with pytest.raises(ValueError, match=rf"\b{bit}\b"):
            R.Generator(3, 3, 4, precision="exact16", n_blocks=1, x2_plan=plan)
    for plan in (0, 7, 59, 97, 283, 763, 1787, 2401):
        assert R._lib.x2_plan_error(plan) is None
        R.Generator(3, 3, 4, precision="exact16", n_blocks=1, x2_plan=plan)
