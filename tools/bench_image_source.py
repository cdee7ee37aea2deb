"""What the whole-image batch sources can feed: the loader twin (`dataset.CropImageDataset` in `DataLoader` workers +
`dataset.CUDAPrefetcher`) at 4 and at 16 workers against the resident source (`device_data.ImageCropSource`), on 64 synthetic
1024 x 768 PNGs written to a temporary directory, batch 16, window 400.

Two measurements, the arms alternated round by round in one process, the figure of an arm the median over the rounds:
  source   batches/s of the source alone: `next()` in a loop (`reset()` at the end of an epoch), wall clock, the device drained
           at the end of the round;
  step     the whole compact `RealESRNetStep` (x4 PReLU, 16 body convs, `fast`, flat fused Adam, GradScaler, EMA; HR crop 256)
           behind `degrade.DegradationPrefetcher` over that source -- the train scripts' loop: ms per step, wall clock.
The yardstick is the loader twin in the same run; both sides and the ratios are recorded, whatever they are.  Nothing is gated on them.

    python tools/bench_image_source.py [--steps 32] [--warmup 8] [--rounds 5] [--out profiles/image_source.jsonl]
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
from real_esrgan_pytorch_amd import config, imgproc  # noqa: E402
from real_esrgan_pytorch_amd.dataset import CropImageDataset, CUDAPrefetcher  # noqa: E402
from real_esrgan_pytorch_amd.degrade import DegradationPrefetcher  # noqa: E402
from real_esrgan_pytorch_amd.device_data import ImageCropSource  # noqa: E402
from real_esrgan_pytorch_amd.train import RealESRNetStep  # noqa: E402

IMAGES, WIDTH, HEIGHT, BATCH, TILE, CROP, S = 64, 1024, 768, 16, 400, 256, 4
ARMS = ("loader4", "loader16", "images")


def write_images(path):
    """Smooth colour fields plus noise: PNGs that cost a real decode."""
    from PIL import Image
    rng = np.random.default_rng(0)
    for i in range(IMAGES):
        low = rng.random((HEIGHT // 8, WIDTH // 8, 3))
        x = 0.8 * np.kron(low, np.ones((8, 8, 1))) + 0.2 * rng.random((HEIGHT, WIDTH, 3))
        Image.fromarray((x * 255).astype(np.uint8)).save(os.path.join(path, f"{i:04d}.png"))


def make_source(arm, path, device):
    if arm == "images":
        return ImageCropSource.from_dir(path, BATCH, TILE, device)
    workers = int(arm[len("loader"):])
    data = CropImageDataset(path, TILE, config.degradation_model_parameters_dict)
    # train_realesrnet.load_dataset's train source.  The workers are spawned, not forked: both loader arms stay alive for the whole
    # run (20 workers), and none of them may inherit the parent's open device; their steady-state rate is the same.
    loader = DataLoader(data, batch_size=BATCH, shuffle=True, num_workers=workers, pin_memory=True, drop_last=True, persistent_workers=True,
                        multiprocessing_context="spawn")
    return CUDAPrefetcher(loader, device)


def make_step():
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=16, upscale=S, act_type="prelu", precision="fast", trainable=True).cuda().train()
    ema = R.EMA(m, 0.999)
    ema.register()
    opt = torch.optim.Adam([m.flat_parameter()], 2e-4, (0.9, 0.99), fused=True)
    return RealESRNetStep(m, ema, opt, torch.amp.GradScaler("cuda"), None)


def run_source(source, count):
    """`count` batches off the source, each touched on the device; seconds of wall clock, the device drained."""
    sink = torch.zeros((), device="cuda")
    t0 = time.perf_counter()
    for _ in range(count):
        batch = source.next()
        if batch is None:
            source.reset()
            batch = source.next()
        sink += batch["hr"][0, 0, 0, 0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_steps(degraded, step, count):
    t0 = time.perf_counter()
    for _ in range(count):
        item = degraded.next()
        if item is None:
            degraded.reset()
            item = degraded.next()
        lr, hr, _ = item
        step(hr, lr)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(line, prefix, run, arms_state, args):
    """The alternated rounds of one measurement: `run(state, count)` seconds -> median and min-max per arm, ratios over loader4."""
    for arm in ARMS:
        run(arms_state[arm], args.warmup)
    times = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            times[arm].append(run(arms_state[arm], args.steps) / args.steps)
    for arm in ARMS:
        med = statistics.median(times[arm])
        line[f"{prefix}_{arm}_ms"] = round(med * 1e3, 3)
        line[f"{prefix}_{arm}_ms_min_max"] = [round(min(times[arm]) * 1e3, 3), round(max(times[arm]) * 1e3, 3)]
        line[f"{prefix}_{arm}_images_per_s"] = round(BATCH / med, 1)
    for arm in ARMS[1:]:
        line[f"{prefix}_{arm}_over_loader4"] = round(statistics.median(times["loader4"]) / statistics.median(times[arm]), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_image_source: needs the MI355X")
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    line = dict(tool="bench_image_source", images=IMAGES, image_size=[WIDTH, HEIGHT], batch=BATCH, tile=TILE, crop=CROP, num_conv=16, precision="fast",
                steps=args.steps, warmup=args.warmup, rounds=args.rounds, yardstick="loader4 (config.num_workers)",
                host_cpus=len(os.sched_getaffinity(0)), device=torch.cuda.get_device_name(0),
                arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    with tempfile.TemporaryDirectory() as path:
        write_images(path)
        t0 = time.perf_counter()
        sources = {"images": make_source("images", path, device)}
        torch.cuda.synchronize()
        line["images_load_s"] = round(time.perf_counter() - t0, 3)      # decode + upload of the whole set, once
        line["arena_bytes"] = int(sources["images"].arena.numel())
        for arm in ARMS[:2]:
            sources[arm] = make_source(arm, path, device)
        # 1. the sources alone
        measure(line, "source", run_source, sources, args)
        # 2. the train loop: degradation one batch ahead, the compact step behind it
        usm, jpeg = imgproc.USMSharp(50, 0).to(device), imgproc.DiffJPEG(False)
        loops = {}
        for arm in ARMS:
            degraded = DegradationPrefetcher(sources[arm], usm, jpeg, S, CROP, device)
            degraded.reset()
            loops[arm] = (degraded, make_step())
        measure(line, "step", lambda loop, count: run_steps(loop[0], loop[1], count), loops, args)
        R._lib.chain_health(sync=True)
        del loops, sources      # the loaders' workers end with their iterators
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
