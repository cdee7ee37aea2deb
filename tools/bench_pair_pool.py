"""What the training pair pool costs: three forms of one exchange at the training step's geometry -- B = 16, Q = 180, LR 3 x 64 x 64,
HR 3 x 256 x 256, fp32, about 150 MB of pool -- and the whole compact training step with the pool off and on.

  exchange  device events around `--steps` exchanges, ms per exchange; the arms alternated round by round in one process, the figure
            of an arm the median over the rounds, with min and max:
              permute  upstream's literal rule in torch: pool = pool[perm], clone the head, assign the head (both tensors);
              index    the slot rule in torch: index_select + index_copy_ on both tensors;
              native   device_data.pool_exchange, one launch (the slots already on the device in every arm: the draw and its upload are
                       the same few bytes for index and native).
  step      the whole compact `RealESRNetStep` (x4 PReLU, 16 body convs, `fast`, flat fused Adam, GradScaler, EMA) fed by the resident
            paired source (`PairedDeviceSource`, 256 synthetic pairs in memory), with the pool off and with `PairPool` on it, full: ms
            per step, wall clock, the device drained at the end of a round.  `PairPool` fills in whole batches and refuses a size that
            the batch does not divide; 180 = 11.25 x 16, so this arm runs at 176, the nearest size it takes (an exchange touches B slots
            whatever Q is).
Nothing is gated on the figures; they are recorded as they come out.

    python tools/bench_pair_pool.py [--steps 50] [--warmup 10] [--rounds 5] [--out profiles/pair_pool.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd import device_data as D  # noqa: E402
from real_esrgan_pytorch_amd.train import RealESRNetStep  # noqa: E402

B, Q, PATCH, S = 16, 180, 64, 4
STEP_Q = Q // B * B      # what `PairPool` takes at this batch size
PAIRS, LR_SIDE = 256, 100
ARMS = ("permute", "index", "native")


class Exchange:
    """The three forms over pools of their own; `slots` / `perm` are drawn per call from a generator of the arm's own."""

    def __init__(self, arm, device):
        g = torch.Generator(device="cpu").manual_seed(0)
        self.arm, self.device = arm, device
        self.pool_lr = torch.rand(Q, 3, PATCH, PATCH, generator=g).to(device)
        self.pool_hr = torch.rand(Q, 3, S * PATCH, S * PATCH, generator=g).to(device)
        self.lr = torch.rand(B, 3, PATCH, PATCH, generator=g).to(device)
        self.hr = torch.rand(B, 3, S * PATCH, S * PATCH, generator=g).to(device)
        self.rng = random.Random(0)

    def draws(self, count):
        """The draws of `count` exchanges, uploaded before the clock starts."""
        if self.arm == "permute":
            return [torch.tensor(self.rng.sample(range(Q), Q), dtype=torch.int64).to(self.device) for _ in range(count)]
        dtype = torch.int32 if self.arm == "native" else torch.int64
        return [torch.from_numpy(D.check_pool_slots(D.sample_pool_slots(self.rng, Q, B), Q, B)).to(dtype).to(self.device) for _ in range(count)]

    def __call__(self, draw):
        if self.arm == "permute":
            self.pool_lr, self.pool_hr = self.pool_lr[draw], self.pool_hr[draw]
            out = (self.pool_lr[:B].clone(), self.pool_hr[:B].clone())
            self.pool_lr[:B] = self.lr
            self.pool_hr[:B] = self.hr
        elif self.arm == "index":
            out = (self.pool_lr.index_select(0, draw), self.pool_hr.index_select(0, draw))
            self.pool_lr.index_copy_(0, draw, self.lr)
            self.pool_hr.index_copy_(0, draw, self.hr)
        else:
            out = D.pool_exchange(self.pool_lr, self.pool_hr, self.lr, self.hr, draw)
        self.lr, self.hr = out      # what came out goes in next: every form keeps moving new data

    def run(self, count):
        draws = self.draws(count)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for d in draws:
            self(d)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / count


def make_source(device):
    rng = np.random.default_rng(0)
    lr = [rng.integers(0, 256, (LR_SIDE, LR_SIDE, 3), dtype=np.uint8) for _ in range(PAIRS)]
    hr = [rng.integers(0, 256, (S * LR_SIDE, S * LR_SIDE, 3), dtype=np.uint8) for _ in range(PAIRS)]
    return D.PairedDeviceSource.from_arrays(hr, lr, B, PATCH, S, device)


def make_step():
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=16, upscale=S, act_type="prelu", precision="fast", trainable=True).cuda().train()
    ema = R.EMA(m, 0.999)
    ema.register()
    opt = torch.optim.Adam([m.flat_parameter()], 2e-4, (0.9, 0.99), fused=True)
    return RealESRNetStep(m, ema, opt, torch.amp.GradScaler("cuda"), None)


def take(source):
    item = source.next()
    if item is None:
        source.reset()
        item = source.next()
    return item


def run_steps(source, step, count):
    t0 = time.perf_counter()
    for _ in range(count):
        lr, hr, _ = take(source)
        step(hr, lr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / count


def record(line, what, times):
    for arm, t in times.items():
        line[f"{what}_{arm}_ms"] = round(statistics.median(t), 4)
        line[f"{what}_{arm}_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pair_pool: needs the MI355X")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    lr_elems, hr_elems = 3 * PATCH * PATCH, 3 * S * S * PATCH * PATCH
    line = dict(tool="bench_pair_pool", batch=B, pool=Q, lr_patch=PATCH, hr_patch=S * PATCH, dtype="float32", pool_bytes=Q * 4 * (lr_elems + hr_elems),
                native_bytes_moved=B * 16 * (lr_elems + hr_elems), step_pool=STEP_Q, num_conv=16, precision="fast", steps=args.steps, warmup=args.warmup,
                rounds=args.rounds, device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    # 1. the exchange alone
    forms = {arm: Exchange(arm, device) for arm in ARMS}
    for arm in ARMS:
        forms[arm].run(args.warmup)
    times = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            times[arm].append(forms[arm].run(args.steps))
    record(line, "exchange", times)
    line["native_gb_per_s"] = round(line["native_bytes_moved"] / (line["exchange_native_ms"] * 1e-3) / 1e9, 1)
    del forms
    # 2. the compact step behind the resident paired source, the pool off and on
    loops = {"pool_off": (make_source(device), make_step())}
    pooled = D.PairPool(make_source(device), STEP_Q, seed=0)
    loops["pool_on"] = (pooled, make_step())
    for arm, (source, step) in loops.items():
        run_steps(source, step, max(args.warmup, STEP_Q // B + 1))      # the pool is full when the rounds start
    assert pooled.filled == STEP_Q
    times = {arm: [] for arm in loops}
    for _ in range(args.rounds):
        for arm, (source, step) in loops.items():
            times[arm].append(run_steps(source, step, args.steps))
    record(line, "step", times)
    line["step_pool_cost_ms"] = round(line["step_pool_on_ms"] - line["step_pool_off_ms"], 4)
    R._lib.chain_health(sync=True)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
