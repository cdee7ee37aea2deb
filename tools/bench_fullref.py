"""What PSNR + SSIM of an SR result against its ground truth cost on the device: the torch backend
(`image_quality_assessment.TorchFullRef`: float64 framework ops, five 11 x 11 conv2ds over full-size maps) against the native path
(`NativeFullRef`, csrc/fullref.hip: two launches) from uint8 frames and from float batches, on

    8k      one 7680 x 4320 image (the x4 result of a 1080p frame)
    16x1k   sixteen 1024 x 1024 images

of smooth colour fields plus grain (seeded); the ground truth is the frame, the result a copy with +-3 levels of noise.  The arms are
alternated round by round in one process; a round is `--calls` calls of one arm between two device events; the figure of an arm is
the median over `--rounds` rounds, its spread their minimum and maximum.  Peak memory is torch.cuda.max_memory_allocated over one call
of the arm, above what the inputs hold.  A last, separate pass times the two native launches one by one (resr_profile_*); the tile
kernel's bytes per second are counted from what it must read once -- 2 x 3 bytes (uint8) or 2 x 12 bytes (float) per pixel -- not from
what the apron makes it read again.  The yardstick is the torch arm of the same run and input kind; every figure is recorded, whatever
it is.  `--native_only` runs the native arms alone (for a kernel trace of its own: rocprofv3 --kernel-trace --stats -- python
tools/bench_fullref.py --native_only).

    python tools/bench_fullref.py [--rounds 5] [--calls 3] [--sizes 8k,16x1k] [--native_only] [--out profiles/fullref.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd.image_quality_assessment import NativeFullRef, TorchFullRef  # noqa: E402

SIZES = {"8k": (1, 4320, 7680), "16x1k": (16, 1024, 1024)}
CROP = 4
TILE_IDS = {34600: "tile_f32_f32", 34601: "tile_u8_f32", 34602: "tile_f32_u8", 34603: "tile_u8_u8"}
FINISH_ID = 34700


def make_pair(b, h, w):
    """(sr, hr) uint8 [b,h,w,3] on the device: hr a smooth field (bicubic from 1/8 size) plus 15 % grain, sr = hr +- 3 levels."""
    g = torch.Generator(device="cuda").manual_seed(0)
    low = torch.rand(b, 3, h // 8, w // 8, device="cuda", generator=g)
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic").clamp_(0, 1).mul_(0.85)
    x.add_(torch.rand(b, 3, h, w, device="cuda", generator=g).mul_(0.15)).clamp_(0, 1)
    hr = (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    del x, low
    noise = torch.randint(-3, 4, hr.shape, device="cuda", generator=g, dtype=torch.int16)
    sr = (hr.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    return sr, hr


def as_float(u8):
    # (divided on the host: one IEEE division per byte, the frame path's (float)byte / 255.0f)
    return (u8.permute(0, 3, 1, 2).cpu().float() / 255.0).contiguous().cuda()


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", default="8k,16x1k")
    ap.add_argument("--native_only", action="store_true", help="skip the torch arms (a kernel trace of the native launches alone)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fullref: needs the MI355X")
    torch.cuda.set_device(0)
    L = R._lib
    native, framework = NativeFullRef(CROP), TorchFullRef(CROP)
    arms = ("native_u8", "native_f32") if args.native_only else ("torch_u8", "torch_f32", "native_u8", "native_f32")
    for size in args.sizes.split(","):
        b, h, w = SIZES[size]
        sr_u8, hr_u8 = make_pair(b, h, w)
        sr_f32, hr_f32 = as_float(sr_u8), as_float(hr_u8)
        calls = {"torch_u8": lambda: framework(sr_u8, hr_u8), "torch_f32": lambda: framework(sr_f32, hr_f32),
                 "native_u8": lambda: native(sr_u8, hr_u8), "native_f32": lambda: native(sr_f32, hr_f32)}
        line = dict(tool="bench_fullref", size=size, batch=b, height=h, width=w, crop_border=CROP, rounds=args.rounds, calls=args.calls,
                    yardstick="torch (TorchFullRef, the same run and input kind)", device=torch.cuda.get_device_name(0),
                    arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], tile=L.RESR_FULLREF_TILE)
        scores = {}
        for arm in arms:                      # warm-up: code objects, the allocator's pools -- and the peak of one call
            calls[arm]()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            scores[arm] = torch.stack(calls[arm]()).cpu()
            line[f"{arm}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        times = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                times[arm].append(timed(calls[arm], args.calls)[0])
        for arm in arms:
            line[f"{arm}_ms"] = round(statistics.median(times[arm]), 3)
            line[f"{arm}_ms_min_max"] = [round(min(times[arm]), 3), round(max(times[arm]), 3)]
        line["psnr_mean_native_u8"], line["ssim_mean_native_u8"] = (float(v) for v in scores["native_u8"].mean(dim=1))
        line["native_u8_equals_native_f32"] = bool(torch.equal(scores["native_u8"], scores["native_f32"]))
        if not args.native_only:
            for kind in ("u8", "f32"):
                t, n = f"torch_{kind}", f"native_{kind}"
                line[f"{t}_over_{n}"] = round(line[f"{t}_ms"] / line[f"{n}_ms"], 2)
                line[f"{n}_beats_torch_beyond_spread"] = bool(max(times[n]) < min(times[t]))
                line[f"{n}_psnr_max_abs_dev"] = float((scores[n][0] - scores[t][0]).abs().max())      # (a near-tie level may round apart: DESIGN)
                line[f"{n}_ssim_max_abs_dev"] = float((scores[n][1] - scores[t][1]).abs().max())
        # the native launches one by one (events around each launch: a pass of its own, after the timing)
        buf = (L.ProfEntry * 64)()
        pixels = b * (h - 2 * CROP) * (w - 2 * CROP)
        for kind, per_pixel in (("u8", 6.0), ("f32", 24.0)):
            L.lib().resr_profile_begin()
            calls[f"native_{kind}"]()
            torch.cuda.synchronize()
            n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), 64))
            entries = [buf[i] for i in range(n)]
            line[f"native_{kind}_launches"] = n
            for e in entries:
                if e.kernel_id in TILE_IDS:
                    line[f"native_{kind}_tile_kernel"] = TILE_IDS[e.kernel_id]
                    line[f"native_{kind}_tile_ms"] = round(e.ms, 4)
                    line[f"native_{kind}_tile_gb_per_s_of_bytes_read_once"] = round(pixels * per_pixel / (e.ms * 1e-3) / 1e9, 1)
                elif e.kernel_id == FINISH_ID:
                    line[f"native_{kind}_finish_ms"] = round(e.ms, 4)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del sr_u8, hr_u8, sr_f32, hr_f32, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
