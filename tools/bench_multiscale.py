"""What the multi-scale copies of the whole-image source cost at start-up: `bench_image_source.py`'s set (64 synthetic 1024 x 768 PNGs),
scales 0.75, 0.5, 1/3 and short side 400 -- 256 copies.  Both arms start from the decoded originals and end with the copies resident,
the device drained:
  pillow    `Image.resize(..., LANCZOS)` of every copy on a thread pool of 16 into one pinned buffer, then one upload;
  resident  `device_data._make_copies` over the resident originals: tables on the thread pool, one upload and one launch per group.
Wall clock, the arms alternated round by round in one process, the figure of an arm the median over the rounds with min-max.  The kernel
alone (resr_resample_u8, all 256 jobs in one launch, tables resident) is timed by device events; its rate is the source plus destination
bytes of the jobs over that time, next to the 6.3 TB/s this part reaches from HBM.  Both arms' copies are compared byte for byte first.
Nothing is gated on the figures.

    python tools/bench_multiscale.py [--rounds 5] [--out profiles/multiscale.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_image_source import HEIGHT, IMAGES, WIDTH, write_images  # noqa: E402
from real_esrgan_pytorch_amd import device_data as D  # noqa: E402

SCALES, SHORT, WORKERS, CHUNK = (0.75, 0.5, 1 / 3), 400, 16, 64 << 20
HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_multiscale: needs the MI355X")
    from PIL import Image
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as path:
        write_images(path)
        originals = [D._read_tile(os.path.join(path, name)) for name in os.listdir(path)]
    M = len(originals)
    table = D._crop_table([a.shape[:2] for a in originals], [str(i) for i in range(M)], D.DEFAULT_MAX_BYTES, SCALES, SHORT)
    first, total = int(table[M, 0]), int(table[-1, 0] + table[-1, 1] * table[-1, 2] * 3)
    arena = torch.empty(total, dtype=torch.uint8, device=device)
    arena[:first].copy_(torch.from_numpy(np.concatenate([a.reshape(-1) for a in originals])))
    pinned = torch.empty(total - first, dtype=torch.uint8).pin_memory()
    images = [Image.fromarray(a) for a in originals]
    line = dict(tool="bench_multiscale", images=IMAGES, image_size=[WIDTH, HEIGHT], scales=[round(s, 4) for s in SCALES], short_side=SHORT, copies=int(table.shape[0] - M),
                original_bytes=first, copy_bytes=total - first, workers=WORKERS, rounds=args.rounds, host_cpus=len(os.sched_getaffinity(0)),
                device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])

    def one_copy(row):
        off, h, w = (int(v) for v in table[row])
        np.copyto(pinned.numpy()[off - first:off - first + h * w * 3].reshape(h, w, 3), np.asarray(images[row % M].resize((w, h), Image.LANCZOS)))

    def pillow_arm(pool):
        list(pool.map(one_copy, range(M, table.shape[0])))
        arena[first:].copy_(pinned, non_blocking=True)

    def resident_arm(pool):
        D._make_copies(arena, table, M, CHUNK, WORKERS)

    def timed(arm, pool):
        arena[first:].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        arm(pool)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    arms = {"pillow": pillow_arm, "resident": resident_arm}
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        results = {}
        for name, arm in arms.items():                                  # warm-up, and the two arms' copies byte for byte
            timed(arm, pool)
            results[name] = arena[first:].clone()
        line["arms_equal"] = bool(torch.equal(results["pillow"], results["resident"]))
        del results
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, arm in arms.items():
                times[name].append(timed(arm, pool))
    for name in arms:
        line[f"{name}_ms"] = round(statistics.median(times[name]) * 1e3, 2)
        line[f"{name}_ms_min_max"] = [round(min(times[name]) * 1e3, 2), round(max(times[name]) * 1e3, 2)]
    line["pillow_over_resident"] = round(statistics.median(times["pillow"]) / statistics.median(times["resident"]), 2)
    # the kernel alone: every copy in one launch, jobs and tables already on the device
    pairs = [(int(table[r % M, 0]), int(table[r % M, 1]), int(table[r % M, 2]), int(table[r, 0]), int(table[r, 1]), int(table[r, 2])) for r in range(M, table.shape[0])]
    jobs, tables = D.resample_jobs(pairs)
    jobs_dev, tables_dev = torch.from_numpy(jobs).to(device), torch.from_numpy(tables).to(device)
    moved = float(sum(h * w * 3 + oh * ow * 3 for _, h, w, _, oh, ow in pairs))
    kernel = []
    for k in range(2 + args.rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        D.resample_u8(arena, jobs, tables_dev, jobs_dev=jobs_dev)
        end.record()
        end.synchronize()
        if k >= 2:
            kernel.append(start.elapsed_time(end) * 1e-3)
    med = statistics.median(kernel)
    line.update(kernel_ms=round(med * 1e3, 3), kernel_ms_min_max=[round(min(kernel) * 1e3, 3), round(max(kernel) * 1e3, 3)], kernel_bytes=moved,
                kernel_GBps=round(moved / med / 1e9, 1), kernel_share_of_hbm=round(moved / med / HBM_ACHIEVABLE, 4), table_bytes=int(tables.size * 4))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
