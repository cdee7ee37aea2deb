"""What the paired data sources can feed: the loader path (`dataset.PairedImageDataset` in `DataLoader` workers + `PairedPrefetcher`) at
4 and at 16 workers against the resident source (`device_data.PairedDeviceSource`), on 256 synthetic pairs written to a temporary
directory -- HR 400 x 400 PNGs with their 100 x 100 partners --, batch 16, LR patch 64 (HR 256), x4.

Two measurements, the arms alternated round by round in one process, the figure of an arm the median over the rounds:
  source   batches/s of the source alone: `next()` in a loop (`reset()` at the end of a pass), wall clock, the device drained at the
           end of the round;
  step     the whole compact `RealESRNetStep` (x4 PReLU, 16 body convs, `fast`, flat fused Adam, GradScaler, EMA) fed by that source
           directly -- the train scripts' loop in the paired modes: ms per step, wall clock.
Nothing is gated on the figures; all arms and the ratios are recorded, whatever they are.  `--arms` leaves arms out (recorded as
"not measured").

    python tools/bench_paired_source.py [--steps 32] [--warmup 8] [--rounds 5] [--arms loader4,loader16,paired] [--out profiles/paired_source.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd.dataset import PairedImageDataset, PairedPrefetcher  # noqa: E402
from real_esrgan_pytorch_amd.device_data import PairedDeviceSource  # noqa: E402
from real_esrgan_pytorch_amd.train import RealESRNetStep  # noqa: E402

PAIRS, HR_SIDE, BATCH, PATCH, S = 256, 400, 16, 64, 4
ARMS = ("loader4", "loader16", "paired")
MAX_CPUS = 16


def write_pairs(path):
    """Smooth colour fields plus noise (PNGs that cost a real decode) and their x4 area means."""
    from PIL import Image
    rng = np.random.default_rng(0)
    hr_dir, lr_dir = os.path.join(path, "hr"), os.path.join(path, "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    for i in range(PAIRS):
        low = rng.random((HR_SIDE // 8, HR_SIDE // 8, 3))
        hr = ((0.8 * np.kron(low, np.ones((8, 8, 1))) + 0.2 * rng.random((HR_SIDE, HR_SIDE, 3))) * 255).astype(np.uint8)
        lr = hr.reshape(HR_SIDE // S, S, HR_SIDE // S, S, 3).mean(axis=(1, 3)).round().astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(hr_dir, f"{i:04d}.png"))
        Image.fromarray(lr).save(os.path.join(lr_dir, f"{i:04d}.png"))
    return hr_dir, lr_dir


def make_source(arm, hr_dir, lr_dir, device):
    if arm == "paired":
        return PairedDeviceSource.from_dirs(hr_dir, lr_dir, BATCH, PATCH, S, device)
    workers = min(int(arm[len("loader"):]), MAX_CPUS)
    data = PairedImageDataset(hr_dir, lr_dir, PATCH, S)
    # train_realesrnet.load_dataset's train source.  The workers are spawned, not forked: both loader arms stay alive for the whole
    # run, and none of them may inherit the parent's open device; their steady-state rate is the same.
    loader = DataLoader(data, batch_size=BATCH, shuffle=True, num_workers=workers, pin_memory=True, drop_last=True, persistent_workers=True,
                        multiprocessing_context="spawn")
    return PairedPrefetcher(loader, device)


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


def run_source(source, count):
    """`count` batches off the source, each touched on the device; seconds of wall clock, the device drained."""
    sink = torch.zeros((), device="cuda")
    t0 = time.perf_counter()
    for _ in range(count):
        lr, hr, _ = take(source)
        sink += hr[0, 0, 0, 0] + lr[0, 0, 0, 0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_steps(source, step, count):
    t0 = time.perf_counter()
    for _ in range(count):
        lr, hr, _ = take(source)
        step(hr, lr)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def record(line, what, times, unit, per_s=None):
    """Median, spread and the ratio to loader4 (where both ran) of every measured arm."""
    for arm, t in times.items():
        med = statistics.median(t)
        line[f"{what}_{arm}_{unit}"] = round(med * 1e3, 3)
        line[f"{what}_{arm}_ms_min_max"] = [round(min(t) * 1e3, 3), round(max(t) * 1e3, 3)]
        if per_s:
            line[f"{what}_{arm}_{per_s}"] = round(1.0 / med, 1)
        if arm != "loader4" and "loader4" in times:
            line[f"{what}_{arm}_over_loader4"] = round(statistics.median(times["loader4"]) / med, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of " + ",".join(ARMS))
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    arms = tuple(a for a in ARMS if a in args.arms.split(","))
    if not arms or set(args.arms.split(",")) - set(ARMS):
        sys.exit(f"bench_paired_source: --arms takes a subset of {ARMS}")
    if not torch.cuda.is_available():
        sys.exit("bench_paired_source: needs the MI355X")
    torch.set_num_threads(min(torch.get_num_threads(), MAX_CPUS))
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    line = dict(tool="bench_paired_source", pairs=PAIRS, hr_side=HR_SIDE, lr_side=HR_SIDE // S, batch=BATCH, lr_patch=PATCH, hr_patch=S * PATCH,
                num_conv=16, precision="fast", steps=args.steps, warmup=args.warmup, rounds=args.rounds, arms=list(arms),
                not_measured=[a for a in ARMS if a not in arms], host_cpus=min(len(os.sched_getaffinity(0)), MAX_CPUS),
                device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    with tempfile.TemporaryDirectory() as path:
        hr_dir, lr_dir = write_pairs(path)
        sources = {}
        for arm in arms:
            t0 = time.perf_counter()
            sources[arm] = make_source(arm, hr_dir, lr_dir, device)
            torch.cuda.synchronize()
            if arm == "paired":
                line["paired_load_s"] = round(time.perf_counter() - t0, 3)      # decode + upload of the whole set, once
        # 1. the sources alone
        for arm in arms:
            run_source(sources[arm], args.warmup)
        times = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                times[arm].append(run_source(sources[arm], args.steps) / args.steps)
        record(line, "source", times, "ms_per_batch", per_s="batches_per_s")
        # 2. the train loop of the paired modes: the compact step fed by the source directly
        loops = {arm: (sources[arm], make_step()) for arm in arms}
        for arm in arms:
            run_steps(*loops[arm], args.warmup)
        times = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                times[arm].append(run_steps(*loops[arm], args.steps) / args.steps)
        record(line, "step", times, "ms")
        R._lib.chain_health(sync=True)
        del loops, sources      # the loaders' workers end with their iterators
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
