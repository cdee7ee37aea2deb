"""CPU: the host side of the training pair pool -- the restated upstream rule ("permute the pool, take its head, overwrite the head")
against the slot rule of `device_data.pool_exchange_np` sample for sample, the fill phase, conservation of uniquely numbered samples,
what `check_pool_slots` and `PairPool` refuse, `config.pair_pool_size`, the declaration of resr_pool_exchange, and the pool's draws
leaving every global generator alone.  `PairPool`'s rule runs here through `HostPairPool`, the same class over CPU tensors."""
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


def _numbered(first, B, lr_shape=(3, 2, 2), hr_shape=(3, 4, 4)):
    """B samples numbered first..first+B-1: every word of sample n's LR side is n, of its HR side n + 0.5."""
    n = np.arange(first, first + B, dtype=np.float32)
    lr = np.ascontiguousarray(np.broadcast_to(n.reshape(-1, 1, 1, 1), (B,) + lr_shape))
    hr = np.ascontiguousarray(np.broadcast_to((n + np.float32(0.5)).reshape(-1, 1, 1, 1), (B,) + hr_shape))
    return lr, hr


def _ids(lr, hr):
    """The numbers of a stack of numbered samples, both sides checked against each other and every word against its sample's number."""
    lr, hr = np.asarray(lr), np.asarray(hr)
    ids = lr.reshape(lr.shape[0], -1)[:, 0]
    assert (lr == ids.reshape(-1, 1, 1, 1)).all() and (hr == (ids + np.float32(0.5)).reshape(-1, 1, 1, 1)).all()
    return [int(i) for i in ids]


class Scripted:
    """A source of the (lr, hr, batch) contract over a list of batches; `device` moves them there."""

    def __init__(self, batches, device=None):
        self.batches, self.device, self.at, self.resets = batches, device, 0, 0

    def reset(self):
        self.resets += 1

    def __len__(self):
        return len(self.batches)

    def next(self):
        if self.at >= len(self.batches):
            return None
        lr, hr = (torch.from_numpy(a.copy()) for a in self.batches[self.at])
        if self.device is not None:
            lr, hr = lr.to(self.device), hr.to(self.device)
        self.at += 1
        return lr, hr, {"lr": lr, "hr": hr, "index": self.at - 1}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_the_slot_rule_hands_out_the_samples_of_upstreams_permutation_rule(D):
    """Rule U (upstream, restated): pool = pool[perm]; out = pool[:B].copy(); pool[:B] = batch.  Rule N: out = pool[slots], pool[slots] =
    batch, the pool never moved.  With `where` carrying U.pool[j] == N.pool[where[j]] (where = where[perm] under the permutation), rule N
    fed slots = where[:B] hands out rule U's samples at every step, in its order, and ends with the same multiset in the pool."""
    Q, B, steps = 12, 4, 40
    rng = np.random.default_rng(3)
    u_lr, u_hr = _numbered(0, Q)
    n_lr, n_hr = u_lr.copy(), u_hr.copy()
    where = np.arange(Q)
    for step in range(steps):
        lr, hr = _numbered(Q + step * B, B)
        perm = rng.permutation(Q)
        u_lr, u_hr, where = u_lr[perm], u_hr[perm], where[perm]
        want = (u_lr[:B].copy(), u_hr[:B].copy())
        u_lr[:B], u_hr[:B] = lr, hr
        got = D.pool_exchange_np(n_lr, n_hr, lr, hr, where[:B])
        assert _ids(*got) == _ids(*want), step
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(u_lr, n_lr[where]) and np.array_equal(u_hr, n_hr[where])      # the invariant holds after the stores
    assert sorted(_ids(u_lr, u_hr)) == sorted(_ids(n_lr, n_hr))
    assert len(set(_ids(n_lr, n_hr))) == Q


def test_exchange_and_store_move_bits_and_only_the_named_slots(D):
    rng = np.random.default_rng(0)
    words = lambda *shape: rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32).view(np.float32)   # NaNs, subnormals
    pool_lr, pool_hr, lr, hr = words(5, 3, 1, 1), words(5, 3, 2, 2), words(2, 3, 1, 1), words(2, 3, 2, 2)
    before = (pool_lr.copy(), pool_hr.copy())
    out_lr, out_hr = D.pool_exchange_np(pool_lr, pool_hr, lr, hr, [4, 1])
    bits = lambda a: a.view(np.int32)
    assert out_lr.dtype == out_hr.dtype == np.float32
    assert np.array_equal(bits(out_lr), bits(before[0])[[4, 1]]) and np.array_equal(bits(out_hr), bits(before[1])[[4, 1]])
    assert np.array_equal(bits(pool_lr)[[4, 1]], bits(lr)) and np.array_equal(bits(pool_hr)[[4, 1]], bits(hr))
    assert np.array_equal(bits(pool_lr)[[0, 2, 3]], bits(before[0])[[0, 2, 3]]) and np.array_equal(bits(pool_hr)[[0, 2, 3]], bits(before[1])[[0, 2, 3]])
    assert D.pool_store_np(pool_lr, pool_hr, out_lr, out_hr, [4, 1]) is None                 # the stores alone put everything back
    assert np.array_equal(bits(pool_lr), bits(before[0])) and np.array_equal(bits(pool_hr), bits(before[1]))
    with pytest.raises(ValueError, match="pool_exchange_np"):
        D.pool_exchange_np(pool_lr, pool_hr, lr, hr[:, :, :1], [0, 1])
    with pytest.raises(ValueError, match="pool_store_np"):
        D.pool_store_np(pool_lr.astype(np.float64), pool_hr, lr, hr, [0, 1])


def test_the_first_q_over_b_batches_come_back_unchanged_and_land_in_order(D):
    Q, B = 12, 4
    batches = [_numbered(k * B, B) for k in range(Q // B + 1)]
    pool = D.HostPairPool(Scripted(batches), Q, seed=5)
    assert pool.filled == 0 and pool.pool_lr is None and len(pool) == len(batches)
    for k in range(Q // B):
        lr, hr, batch = pool.next()
        assert _ids(lr, hr) == list(range(k * B, (k + 1) * B)) and batch["index"] == k and batch["lr"] is lr and batch["hr"] is hr
        assert pool.filled == (k + 1) * B
        assert _ids(pool.pool_lr[:pool.filled], pool.pool_hr[:pool.filled]) == list(range(pool.filled))      # slots ptr..ptr+B-1
    assert tuple(pool.pool_lr.shape) == (Q, 3, 2, 2) and tuple(pool.pool_hr.shape) == (Q, 3, 4, 4) and pool.pool_lr.dtype == torch.float32
    lr, hr, batch = pool.next()                                         # full: the first exchange
    slots = random.Random(5).sample(range(Q), B)                        # sample_pool_slots, typed out
    assert _ids(lr, hr) == slots and batch["index"] == Q // B           # slot s held sample s; the dictionary is the incoming batch's
    assert _ids(batch["lr"], batch["hr"]) == list(range(Q, Q + B))
    assert [_ids(pool.pool_lr, pool.pool_hr)[s] for s in slots] == list(range(Q, Q + B)) and pool.filled == Q
    assert pool.next() is None and pool.next() is None                  # the source's end is the pool's; nothing is drained
    assert pool.filled == Q


def test_every_sample_that_entered_is_handed_out_or_in_the_pool_exactly_once(D):
    Q, B = 12, 4
    steps = 3 * Q // B
    pool = D.HostPairPool(Scripted([_numbered(k * B, B) for k in range(steps)]), Q, seed=1)
    out = []
    for _ in range(steps):
        lr, hr, _batch = pool.next()
        out.append(_ids(lr, hr))
    fill = Q // B
    assert out[:fill] == [list(range(k * B, (k + 1) * B)) for k in range(fill)]          # the fill hands the batches themselves out ...
    exchanged = [i for ids in out[fill:] for i in ids]
    left = _ids(pool.pool_lr, pool.pool_hr)
    assert sorted(exchanged + left) == list(range(steps * B))           # ... and from then on: handed out + in the pool = what entered, once each
    assert exchanged != sorted(exchanged)                               # and not in the order of entry


def test_reset_and_attach_keep_the_contents_and_the_fill_pointer(D):
    first = Scripted([_numbered(0, 2), _numbered(2, 2)])
    pool = D.HostPairPool(first, 8, seed=0)
    pool.next()
    pool.next()
    assert pool.next() is None and pool.filled == 4
    pool.reset()
    assert first.resets == 1 and pool.filled == 4 and _ids(pool.pool_lr[:4], pool.pool_hr[:4]) == [0, 1, 2, 3]
    second = Scripted([_numbered(10, 2), _numbered(12, 2), _numbered(14, 2)])
    second.original_dataloader = "the loader"
    with pytest.raises(AttributeError):
        pool.original_dataloader                                        # the first source has none
    pool.attach(second)
    assert pool.source is second and pool.original_dataloader == "the loader" and len(pool) == 3
    pool.next()
    pool.next()
    assert pool.filled == 8 and _ids(pool.pool_lr, pool.pool_hr) == [0, 1, 2, 3, 10, 11, 12, 13]
    lr, hr, _batch = pool.next()
    assert set(_ids(lr, hr)) <= {0, 1, 2, 3, 10, 11, 12, 13}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_check_pool_slots_refuses_a_repeat_a_slot_out_of_range_and_a_wrong_count_by_name(D):
    out = D.check_pool_slots([5, 0, 11, 3], 12, 4)
    assert out.dtype == np.int32 and out.tolist() == [5, 0, 11, 3] and out.flags["C_CONTIGUOUS"]
    assert D.check_pool_slots(np.arange(4)[::-1], 4, 4).tolist() == [3, 2, 1, 0]                 # Q = B: every slot
    for slots, word in (([5, 0, 5, 3], r"slot 5 repeated \(entries 0 and 2\)"), ([5, 0, 12, 3], r"slot 12 of entry 2 outside 0\.\.11"),
                        ([5, -1, 11, 3], r"slot -1 of entry 1 outside 0\.\.11"), ([5, 0, 11], "expected 4 integer slots"),
                        ([5, 0, 11, 3, 4], "expected 4 integer slots"), ([5.0, 0.0, 11.0, 3.0], "expected 4 integer slots"),
                        ([[5, 0], [11, 3]], "expected 4 integer slots")):
        with pytest.raises(ValueError, match="pool slots: " + word):
            D.check_pool_slots(slots, 12, 4)
    rng = random.Random(9)
    for _ in range(50):
        slots = D.sample_pool_slots(rng, 12, 4)
        assert len(set(slots)) == 4 and D.check_pool_slots(slots, 12, 4).tolist() == slots


def test_pair_pool_refuses_a_bad_size_before_any_allocation(D):
    batches = [_numbered(0, 4)]
    for size, kwargs, word in ((10, {}, "size 10 is not a multiple of the batch size 4"), (2, {}, "size 2 below the batch size 4"),
                               (8, dict(max_bytes=8 * 4 * (12 + 48) - 1), "1920 bytes, above max_bytes=1919")):
        pool = D.HostPairPool(Scripted(batches), size, **kwargs)
        with pytest.raises(ValueError, match="pair pool: .*" + word):
            pool.next()
        assert pool.pool_lr is None and pool.pool_hr is None and pool.filled == 0
    with pytest.raises(ValueError, match="size 0"):
        D.PairPool(Scripted(batches), 0)
    pool = D.HostPairPool(Scripted(batches), 8, max_bytes=8 * 4 * (12 + 48))             # exactly the budget is taken
    assert pool.next() is not None and pool.filled == 4
    pool.attach(Scripted([_numbered(0, 4, lr_shape=(3, 3, 3))]))
    with pytest.raises(ValueError, match="after the pool was sized"):
        pool.next()
    pool.attach(Scripted([_numbered(0, 2)]))                            # another batch size is another shape
    with pytest.raises(ValueError, match="after the pool was sized"):
        pool.next()
    assert D.POOL_DEFAULT_MAX_BYTES == 8 << 30
    with pytest.raises(RuntimeError, match="PairPool: expected a tensor on the MI355X device"):      # the device pool has no CPU path
        D.PairPool(Scripted(batches), 8).next()


# ---- random state --------------------------------------------------------------------------------------------------------------------
def test_the_pools_draws_leave_every_global_generator_untouched(D):
    random.seed(4)
    np.random.seed(4)
    torch.manual_seed(4)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    Q, B = 8, 4
    pool = D.HostPairPool(Scripted([_numbered(k * B, B) for k in range(6)]), Q, seed=2)
    seen = []
    while True:
        item = pool.next()
        if item is None:
            break
        seen.append(_ids(item[0], item[1]))
    assert len(seen) == 6 and seen[2:] != [list(range(k * B, (k + 1) * B)) for k in range(2, 6)]      # four exchanges were drawn
    now = np.random.get_state()
    assert random.getstate() == before[0]
    assert now[0] == before[1][0] and np.array_equal(now[1], before[1][1]) and now[2:] == before[1][2:]
    assert torch.equal(torch.get_rng_state(), before[2])
    again = D.HostPairPool(Scripted([_numbered(k * B, B) for k in range(6)]), Q, seed=2)
    assert [_ids(*again.next()[:2]) for _ in range(6)] == seen          # the pool's sequence is its seed's
    other = D.HostPairPool(Scripted([_numbered(k * B, B) for k in range(6)]), Q, seed=3)
    assert [_ids(*other.next()[:2]) for _ in range(6)] != seen          # another rank's seed, other slots


# ---- the header ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_resr_pool_exchange_once_and_the_library_exports_it(D):
    import ctypes as C
    from real_esrgan_pytorch_amd import _lib
    text = open(os.path.join(ROOT, "include", "resr.h")).read()
    assert len(re.findall(r"\bint resr_pool_exchange\(", text)) == 1
    assert "resr_pool_exchange" in _lib.exported_symbols()
    res, args = _lib._PROTOS["resr_pool_exchange"]
    assert res is C.c_int and len(args) == 12 and args[9] is C.c_int64 and args[10] is C.c_int64
    assert callable(C.CDLL(_lib.LIB_PATH).resr_pool_exchange)           # the built library itself, not the binding's table
    assert callable(_lib.lib().resr_pool_exchange)
    api = open(os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "host_api.h")).read()
    assert len(re.findall(r"\bint pool_exchange_dispatch\(", api)) == 1


# ---- config --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def config(D, monkeypatch):
    from real_esrgan_pytorch_amd import config as module
    state = (torch.get_rng_state(), random.getstate(), np.random.get_state())

    def reload(pool=None, mode=None):
        for name, value in (("RESR_PAIR_POOL", pool), ("RESR_MODE", mode)):
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


def test_config_reads_the_pool_size_and_refuses_what_cannot_fill_in_whole_batches(config, monkeypatch):
    c = config()
    assert c.pair_pool_size == 0 and c.pair_pool() == 0                 # off by default
    c = config("180", "test")                                           # upstream's value; outside a training mode no batch size binds it
    assert c.pair_pool_size == 180
    for mode in ("train_realesrnet", "train_realesrgan"):
        c = config("192", mode)
        assert c.pair_pool_size == 192 and c.batch_size == 48 and c.pair_pool() == 192
        with pytest.raises(ValueError, match="pair_pool_size=180.*not a multiple of batch_size=48"):
            config("180", mode)
        with pytest.raises(ValueError, match="RESR_PAIR_POOL=-48"):
            config("-48", mode)
    with pytest.raises(ValueError, match="RESR_PAIR_POOL=-1"):
        config("-1", "test")
    c = config("192")
    monkeypatch.setattr(c, "batch_size", 12)                            # upstream's own geometry: 180 = 15 batches of 12
    monkeypatch.setattr(c, "pair_pool_size", 180)
    assert c.pair_pool() == 180
    monkeypatch.setattr(c, "batch_size", 16)
    with pytest.raises(ValueError, match="not a multiple of batch_size=16"):
        c.pair_pool()


def test_train_pairs_wraps_its_source_in_one_pool_per_process(D, monkeypatch):
    """With the pool off train_pairs returns what it returned before; with it on, one `PairPool` per process, re-attached to each
    epoch's source; a size that the batch does not divide is refused there too."""
    from real_esrgan_pytorch_amd import config
    from real_esrgan_pytorch_amd import train_realesrnet as T
    monkeypatch.setattr(config, "data_source", "paired")
    monkeypatch.setattr(config, "batch_size", 4)
    monkeypatch.setattr(T, "_PAIR_POOL", None)
    a, b = Scripted([]), Scripted([])
    assert T.train_pairs(a) is a and T._PAIR_POOL is None               # pair_pool_size = 0
    monkeypatch.setattr(config, "pair_pool_size", 8)
    monkeypatch.setattr(T, "_RANK", 3)
    pool = T.train_pairs(a)
    assert isinstance(pool, D.PairPool) and pool.source is a and pool.size == 8 and T._PAIR_POOL is pool
    assert pool._rng.getstate() == random.Random(3).getstate()          # seeded with the rank
    assert T.train_pairs(b) is pool and pool.source is b                # the next epoch: the same pool over the new source
    monkeypatch.setattr(config, "pair_pool_size", 10)
    with pytest.raises(ValueError, match="not a multiple of batch_size=4"):
        T.train_pairs(a)
