"""-m gpu: resr_pool_exchange against its definition, device_data.pool_exchange_np / pool_store_np, bit for bit -- compared as int32:
the kernel moves 32-bit words and the payload is random bit patterns, NaNs and subnormals among them, so there is no tolerance
anywhere.  Shapes: sample sizes that are and are not multiples of 4 floats (3 P^2 with P odd starts every sample but the first off a
16-byte boundary), tails shorter than a chunk, more than one chunk, Q = B (every slot exchanged) and Q > B (the slots not named keep
their bits), shuffled slots, base pointers off 16 bytes under a vector-sized sample, the store-only and the in-place forms, a pool past
byte 2^31 and every refusal.  Every tensor stands between guard words that must keep their bits.

Only legal slots reach the GPU here: the kernel's clamp of a slot is a safety net that stays unexercised, and what refuses a wrong slot,
device_data.check_pool_slots, is tested on the CPU (tests/test_pair_pool_surface.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POOL_EXCHANGE_ID = 33002
GUARD = 64
SENT = 0x7FC5A5A5      # a NaN payload, as int32


@pytest.fixture(scope="module")
def D():
    from real_esrgan_pytorch_amd import device_data
    return device_data


@pytest.fixture(scope="module")
def L():
    from real_esrgan_pytorch_amd import _lib
    return _lib


def _launches(L, fn):
    lib = L.lib()
    lib.resr_profile_begin()
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), 64))
    return [(buf[i].kernel_id, buf[i].bytes) for i in range(n)]


class Guarded:
    """int32 words on the device between two guards of GUARD sentinel words; `shift` words of sentinel more in front, so that the
    payload starts 4 * shift bytes off the allocation's alignment."""

    def __init__(self, words, shift=0):
        self.words = np.ascontiguousarray(words, dtype=np.int32)
        self.count, self.front = self.words.size, GUARD + shift
        host = np.full(self.front + self.count + GUARD, SENT, dtype=np.int32)
        host[self.front:self.front + self.count] = self.words.reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = C.c_void_p(self.t.data_ptr() + 4 * self.front)

    def read(self):
        a = self.t.cpu().numpy()
        assert (a[:self.front] == SENT).all(), "the guard in front was written"
        assert (a[self.front + self.count:] == SENT).all(), "the guard behind was written"
        return a[self.front:self.front + self.count].reshape(self.words.shape)


def _words(rng, *shape):
    """Random 32-bit patterns, with a NaN, an infinity, a subnormal and a negative zero planted at the front of every sample."""
    a = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    flat = a.reshape(shape[0], -1)
    special = np.array([0x7FC00001, 0x7F800000, 0x00000001, -2 ** 31], dtype=np.int64).astype(np.int32)
    flat[:, :min(4, flat.shape[1])] = special[:flat.shape[1]]
    return a


def _case(P, scale, Q, B, seed):
    rng = np.random.default_rng(seed)
    lr_shape, hr_shape = (3, P, P), (3, scale * P, scale * P)
    slots = rng.permutation(Q)[:B].astype(np.int32)                     # B different slots in a shuffled order
    if B > 1 and (np.diff(slots) > 0).all():
        slots = slots[::-1].copy()
    return _words(rng, Q, *lr_shape), _words(rng, Q, *hr_shape), _words(rng, B, *lr_shape), _words(rng, B, *hr_shape), slots


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def _call(L, pool_lr, pool_hr, lr, hr, out_lr, out_hr, slots, Q, B, lr_elems, hr_elems):
    return L.lib().resr_pool_exchange(pool_lr, pool_hr, lr, hr, out_lr, out_hr, slots, Q, B, lr_elems, hr_elems, L.stream_ptr())


def _run(D, L, P, scale, Q, B, mode="exchange", shift=(0, 0, 0), seed=0):
    """One launch over guarded tensors against the definition.  mode: "exchange", "store" (null outputs) or "alias" (out is in);
    shift: words that the pools, the inputs and the outputs start off a 16-byte boundary."""
    pool_lr, pool_hr, lr, hr, slots = _case(P, scale, Q, B, seed)
    want_pool = (_f32(pool_lr.copy()), _f32(pool_hr.copy()))
    if mode == "store":
        D.pool_store_np(want_pool[0], want_pool[1], _f32(lr), _f32(hr), slots)
        want_out = None
    else:
        want_out = D.pool_exchange_np(want_pool[0], want_pool[1], _f32(lr), _f32(hr), slots)
    g_pool = (Guarded(pool_lr, shift[0]), Guarded(pool_hr, shift[0]))
    g_in = (Guarded(lr, shift[1]), Guarded(hr, shift[1]))
    g_out = (Guarded(np.full_like(lr, SENT), shift[2]), Guarded(np.full_like(hr, SENT), shift[2]))
    s_dev = torch.from_numpy(slots).cuda()
    outs = {"exchange": (g_out[0].ptr, g_out[1].ptr), "store": (None, None), "alias": (g_in[0].ptr, g_in[1].ptr)}[mode]
    lr_elems, hr_elems = 3 * P * P, 3 * scale * scale * P * P
    seen = _launches(L, lambda: L.check(_call(L, g_pool[0].ptr, g_pool[1].ptr, g_in[0].ptr, g_in[1].ptr, outs[0], outs[1], L.ptr(s_dev), Q, B,
                                              lr_elems, hr_elems), "resr_pool_exchange"))
    moved = B * (lr_elems + hr_elems) * (8 if mode == "store" else 16)  # bytes read + bytes written
    assert seen == [(POOL_EXCHANGE_ID, float(moved))], seen             # ONE launch moves both tensors, under its profiling id
    for side, name in ((0, "lr"), (1, "hr")):
        got_pool = g_pool[side].read()
        assert np.array_equal(got_pool, want_pool[side].view(np.int32)), (name, "pool")      # the slots not named kept their bits too
        handed = g_out[side].read()
        kept = g_in[side].read()
        if mode == "exchange":
            assert np.array_equal(handed, want_out[side].view(np.int32)), (name, "out")
            assert np.array_equal(kept, (lr, hr)[side]), (name, "the input was written")
        elif mode == "alias":
            assert np.array_equal(kept, want_out[side].view(np.int32)), (name, "in place")
            assert (handed == SENT).all()
        else:
            assert (handed == SENT).all() and np.array_equal(kept, (lr, hr)[side]), (name, "store only")
    return slots


@pytest.mark.parametrize("Q", [3, 9])
@pytest.mark.parametrize("scale", [1, 2, 3, 4])
@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 33])
def test_pool_exchange_is_pool_exchange_np_bit_for_bit(D, L, P, scale, Q):
    slots = _run(D, L, P, scale, Q, 3, seed=1000 * P + 10 * scale + Q)
    assert len(set(slots.tolist())) == 3 and slots.tolist() != sorted(slots.tolist())
    if Q == 3:
        assert sorted(slots.tolist()) == [0, 1, 2]                      # Q = B: every slot is exchanged


@pytest.mark.parametrize("P,scale", [(5, 2), (8, 4), (33, 1)])
def test_null_outputs_store_only(D, L, P, scale):
    _run(D, L, P, scale, 9, 3, mode="store", seed=P)


@pytest.mark.parametrize("P,scale", [(5, 2), (8, 4), (33, 1)])
def test_an_output_that_is_its_input_swaps_in_place(D, L, P, scale):
    _run(D, L, P, scale, 9, 3, mode="alias", seed=P + 1)


@pytest.mark.parametrize("shift", [(1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 1, 1)])
def test_a_base_pointer_off_16_bytes_takes_the_scalar_form_with_the_same_result(D, L, shift):
    """3 * 8^2 and 3 * 32^2 floats are multiples of 4, so only the pointers decide here; (1, 1, 1) keeps every tensor 4 bytes off."""
    _run(D, L, 8, 4, 9, 3, shift=shift, seed=sum(shift))
    if shift == (0, 2, 0):
        _run(D, L, 8, 4, 9, 3, mode="alias", shift=shift, seed=7)
        _run(D, L, 8, 4, 9, 3, mode="store", shift=shift, seed=8)


def test_the_python_wrappers_move_the_same_bits_and_refuse_what_is_not_a_pool(D):
    pool_lr, pool_hr, lr, hr, slots = _case(5, 3, 7, 4, 42)
    want_pool = (_f32(pool_lr.copy()), _f32(pool_hr.copy()))
    want_out = D.pool_exchange_np(want_pool[0], want_pool[1], _f32(lr), _f32(hr), slots)
    dev = lambda a: torch.from_numpy(_f32(a).copy()).cuda()
    bits = lambda t: t.cpu().numpy().view(np.int32)
    t_pool, t_in, s_dev = (dev(pool_lr), dev(pool_hr)), (dev(lr), dev(hr)), torch.from_numpy(slots).cuda()
    out = D.pool_exchange(t_pool[0], t_pool[1], t_in[0], t_in[1], s_dev)
    torch.cuda.synchronize()
    for side in (0, 1):
        assert out[side].shape == t_in[side].shape and out[side].data_ptr() != t_in[side].data_ptr()
        assert np.array_equal(bits(out[side]), want_out[side].view(np.int32)) and np.array_equal(bits(t_pool[side]), want_pool[side].view(np.int32))
    back = D.pool_exchange(t_pool[0], t_pool[1], out[0], out[1], s_dev, out=out)      # in place: the first exchange undone
    assert back[0] is out[0] and back[1] is out[1]
    torch.cuda.synchronize()
    for side, (pool, batch) in enumerate(((pool_lr, lr), (pool_hr, hr))):
        assert np.array_equal(bits(t_pool[side]), pool) and np.array_equal(bits(out[side]), batch)
    assert D.pool_store(t_pool[0], t_pool[1], t_in[0], t_in[1], s_dev) is None
    torch.cuda.synchronize()
    D.pool_store_np(_f32(pool_lr), _f32(pool_hr), _f32(lr), _f32(hr), slots)
    assert np.array_equal(bits(t_pool[0]), pool_lr) and np.array_equal(bits(t_pool[1]), pool_hr)
    p_lr, p_hr, b_lr, b_hr = t_pool[0], t_pool[1], t_in[0], t_in[1]
    for args in ((p_lr.double(), p_hr, b_lr, b_hr, s_dev), (p_lr, p_hr[:, :, :, :3], b_lr, b_hr, s_dev), (p_lr, p_hr, b_lr[:, :, :4], b_hr, s_dev),
                 (p_lr, p_hr, b_lr[:3], b_hr, s_dev), (p_lr, p_hr[:6], b_lr, b_hr, s_dev), (p_lr, p_hr, b_lr, b_hr, s_dev.long()),
                 (p_lr, p_hr, b_lr, b_hr, s_dev[:3]), (p_lr, p_hr, b_lr.cpu(), b_hr, s_dev), (p_lr, p_hr, b_lr, b_hr, s_dev.cpu())):
        with pytest.raises(ValueError, match="pool_exchange"):
            D.pool_exchange(*args)
    with pytest.raises(ValueError, match="pool_store"):
        D.pool_store(p_lr, p_hr, b_lr, b_hr.half(), s_dev)
    with pytest.raises(ValueError, match="pool_exchange: out"):
        D.pool_exchange(p_lr, p_hr, b_lr, b_hr, s_dev, out=(b_lr, b_lr))
    with pytest.raises(RuntimeError, match="RESR_ERR_ARG|overlap"):     # the library's own refusal reaches Python: the input lies in the pool
        D.pool_exchange(p_lr, p_hr, p_lr[:4], b_hr, s_dev)


def test_a_pool_past_2_31_bytes_exchanges_its_last_slot(D):
    """HR samples of 3 * 256^2 floats, Q = 2731: 2,147,745,792 bytes of pool, the last slot running from byte 2^31 - 524,288 across
    2^31 to the end -- a 32-bit byte offset wraps inside it.  The pool is zeros on the device; no host array of that size is made."""
    Q, B, hr_elems = 2731, 2, 3 * 256 * 256
    assert (Q - 1) * hr_elems * 4 < 2 ** 31 < Q * hr_elems * 4
    rng = np.random.default_rng(11)
    pool_hr = torch.zeros(Q, 3, 256, 256, dtype=torch.float32, device="cuda")
    pool_lr = torch.zeros(Q, 3, 1, 1, dtype=torch.float32, device="cuda")
    last = torch.from_numpy(_f32(_words(rng, 1, 3, 256, 256))).cuda()
    pool_hr[Q - 1] = last[0]
    pool_lr[Q - 1] = 5.0
    hr = torch.from_numpy(_f32(_words(rng, B, 3, 256, 256))).cuda()
    lr = torch.from_numpy(_f32(_words(rng, B, 3, 1, 1))).cuda()
    slots = torch.tensor([Q - 1, 1], dtype=torch.int32, device="cuda")
    out_lr, out_hr = D.pool_exchange(pool_lr, pool_hr, lr, hr, slots)
    torch.cuda.synchronize()
    i32 = lambda t: t.view(torch.int32)
    assert torch.equal(i32(out_hr[0]), i32(last[0])) and torch.equal(i32(pool_hr[Q - 1]), i32(hr[0]))
    assert torch.equal(i32(pool_hr[1]), i32(hr[1])) and int(i32(out_hr[1]).abs().max()) == 0
    assert float(out_lr[0].min()) == float(out_lr[0].max()) == 5.0 and torch.equal(i32(pool_lr[Q - 1]), i32(lr[0])) and torch.equal(i32(pool_lr[1]), i32(lr[1]))
    for untouched in (0, 2, Q - 2):
        assert int(i32(pool_hr[untouched]).abs().max()) == 0 and int(i32(pool_lr[untouched]).abs().max()) == 0


def test_refusals_come_before_any_launch(D, L):
    P, scale, Q, B = 4, 2, 4, 2
    lr_elems, hr_elems = 3 * P * P, 3 * scale * scale * P * P
    pool_lr, pool_hr, lr, hr, slots = _case(P, scale, Q, B, 5)
    g = dict(pool_lr=Guarded(pool_lr), pool_hr=Guarded(pool_hr), lr=Guarded(lr), hr=Guarded(hr), out_lr=Guarded(np.full_like(lr, SENT)),
             out_hr=Guarded(np.full_like(hr, SENT)))
    s_dev = torch.from_numpy(slots).cuda()
    at = lambda name, words=0: C.c_void_p(g[name].ptr.value + 4 * words)
    ok = dict(pool_lr=at("pool_lr"), pool_hr=at("pool_hr"), lr=at("lr"), hr=at("hr"), out_lr=at("out_lr"), out_hr=at("out_hr"), slots=L.ptr(s_dev),
              q=Q, b=B, lr_elems=lr_elems, hr_elems=hr_elems)
    cases = [dict(pool_lr=None), dict(pool_hr=None), dict(lr=None), dict(hr=None), dict(slots=None),
             dict(out_lr=None), dict(out_hr=None),                      # exactly one null output
             dict(q=0), dict(q=-4), dict(b=0), dict(b=-1), dict(lr_elems=0), dict(lr_elems=-48), dict(hr_elems=0), dict(hr_elems=-1),
             dict(b=3, q=2), dict(b=Q + 1),                             # B > Q
             dict(b=65536, q=65536), dict(b=65536, q=2 ** 31 - 1),      # the grid's y dimension
             dict(lr_elems=2 ** 43), dict(hr_elems=2 ** 43), dict(lr_elems=2 ** 42, hr_elems=2 ** 42), dict(lr_elems=2 ** 62, hr_elems=2 ** 62),
             dict(hr_elems=2 ** 63 - 1),                                # the grid: 2^31 chunks of 4096 words and more
             dict(lr=at("pool_lr")), dict(lr=at("pool_lr", (Q - 1) * lr_elems + lr_elems - 1)), dict(hr=at("pool_hr", hr_elems)),      # the input in the pool
             dict(out_lr=at("pool_lr", lr_elems)), dict(out_hr=at("pool_hr")),                                                     # the output in the pool
             dict(out_lr=at("lr", 1)), dict(out_lr=at("lr", lr_elems)), dict(out_hr=at("hr", B * hr_elems - 1)),                      # output and input overlap, not equal
             dict(pool_lr=at("lr", -(Q * lr_elems - 1))), dict(pool_hr=at("out_hr", B * hr_elems - 1))]                               # one word shared

    def call(a):
        return _call(L, a["pool_lr"], a["pool_hr"], a["lr"], a["hr"], a["out_lr"], a["out_hr"], a["slots"], a["q"], a["b"], a["lr_elems"], a["hr_elems"])
    answers = []

    def refused():
        for change in cases:
            answers.append((change, call(dict(ok, **change)), L.lib().resr_last_error()))
    seen = _launches(L, refused)
    for change, rc, text in answers:
        assert rc == L.RESR_ERR_ARG and b"pool_exchange" in text, (change, rc, text)
    assert len(answers) == len(cases) and seen == []                    # no profiling record: nothing of id 33002 (or any id) was launched
    for name, words in (("pool_lr", pool_lr), ("pool_hr", pool_hr), ("lr", lr), ("hr", hr)):
        assert np.array_equal(g[name].read(), words), name              # and nothing was written
    assert (g["out_lr"].read() == SENT).all() and (g["out_hr"].read() == SENT).all()
    # the arguments the cases start from do run, and so do the two legal forms next to the refused ones
    for change in ({}, dict(out_lr=None, out_hr=None), dict(out_lr=at("lr"), out_hr=at("hr"))):
        assert [i for i, _ in _launches(L, lambda: L.check(call(dict(ok, **change)), "resr_pool_exchange"))] == [POOL_EXCHANGE_ID], change
    for name in g:
        g[name].read()                                                  # the guards still stand
