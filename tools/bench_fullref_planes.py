"""What PSNR + SSIM per plane cost on the device (csrc/fullref.hip, resr_fullref_planes), on the two inputs of tools/bench_fullref.py

    8k      one 7680 x 4320 image (the x4 result of a 1080p frame)
    16x1k   sixteen 1024 x 1024 images

RGB arms, a uint8 [B,H,W,3] pair: `full_ref_channels_native` (one call, two launches for the batch and the three channels) against its
torch float64 twin `full_ref_channels` on the device.  YUV arms, the same pair as i420 frames (`rgb_to_yuv420`, outside the timing):
`full_ref_yuv_native` (two calls, four launches: the stored Y, Cb and Cr planes) against what scoring a frame took before it --
`yuv420_to_rgb` and `full_ref_native` on the result (three launches: the BT.601 luma level of the frame's RGB, another quantity, and no
chroma numbers).  The arms are alternated round by round in one process; a round is `--calls` calls of one arm between two device
events; the figure of an arm is the median over `--rounds` rounds, its spread their minimum and maximum.  Peak memory is
torch.cuda.max_memory_allocated over one call of the arm, above what the inputs hold.  A last, separate pass times the native launches
one by one (resr_profile_*); the tile kernel's bytes per second are counted from what it must read once, 2 bytes per sample.  Nothing
is gated on these times; every figure is recorded, whatever it is.

    python tools/bench_fullref_planes.py [--rounds 5] [--calls 3] [--sizes 8k,16x1k] [--native_only] [--out profiles/fullref_planes.jsonl]
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
from real_esrgan_pytorch_amd import frames as Fr  # noqa: E402
from real_esrgan_pytorch_amd import image_quality_assessment as Q  # noqa: E402
from bench_fullref import SIZES, make_pair, timed  # noqa: E402  (tools/ is the script's directory)

CROP = 4
TILE_ID, FINISH_ID = 34604, 34701


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", default="8k,16x1k")
    ap.add_argument("--native_only", action="store_true", help="skip the torch twin (a kernel trace of the native launches alone)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fullref_planes: needs the MI355X")
    torch.cuda.set_device(0)
    L = R._lib
    arms = ("rgb_native", "yuv_native", "yuv_via_rgb") + (() if args.native_only else ("rgb_torch",))
    for size in args.sizes.split(","):
        b, h, w = SIZES[size]
        sr, hr = make_pair(b, h, w)
        sr_yuv, hr_yuv = Fr.rgb_to_yuv420(sr), Fr.rgb_to_yuv420(hr)
        calls = {"rgb_native": lambda: Q.full_ref_channels_native(sr, hr, CROP)[3:],
                 "rgb_torch": lambda: Q.full_ref_channels(sr, hr, CROP)[3:],
                 "yuv_native": lambda: Q.full_ref_yuv_native(sr_yuv, hr_yuv, "i420", None, CROP),
                 "yuv_via_rgb": lambda: Q.full_ref_native(Fr.yuv420_to_rgb(sr_yuv), Fr.yuv420_to_rgb(hr_yuv), CROP)}
        line = dict(tool="bench_fullref_planes", size=size, batch=b, height=h, width=w, crop_border=CROP, rounds=args.rounds, calls=args.calls,
                    yardsticks={"rgb_native": "rgb_torch (full_ref_channels, the same run)", "yuv_native": "yuv_via_rgb (yuv420_to_rgb of both sides + full_ref_native, the same run)"},
                    device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], tile=L.RESR_FULLREF_TILE)
        scores = {}
        for arm in arms:                      # warm-up: code objects, the allocator's pools -- and the peak of one call
            try:
                calls[arm]()
            except torch.cuda.OutOfMemoryError:     # the float64 twin of three 8K channels may not fit beside other work: recorded, not timed
                line[f"{arm}_error"] = "out of memory"
                torch.cuda.empty_cache()
                continue
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            scores[arm] = torch.stack(list(calls[arm]())).cpu()
            line[f"{arm}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        ran = [arm for arm in arms if arm in scores]
        times = {arm: [] for arm in ran}
        for _ in range(args.rounds):
            for arm in ran:
                times[arm].append(timed(calls[arm], args.calls)[0])
        for arm in ran:
            line[f"{arm}_ms"] = round(statistics.median(times[arm]), 3)
            line[f"{arm}_ms_min_max"] = [round(min(times[arm]), 3), round(max(times[arm]), 3)]
        line["rgb_psnr_all_mean"], line["rgb_ssim_mean_mean"] = (float(v) for v in scores["rgb_native"].mean(dim=1))
        line["yuv_psnr_y_u_v_avg_mean"] = [float(v) for v in scores["yuv_native"][:4].mean(dim=1)]
        line["yuv_ssim_y_u_v_mean"] = [float(v) for v in scores["yuv_native"][4:].mean(dim=1)]
        line["via_rgb_psnr_ssim_mean"] = [float(v) for v in scores["yuv_via_rgb"].mean(dim=1)]
        pairs = [("yuv_via_rgb", "yuv_native")] + ([("rgb_torch", "rgb_native")] if "rgb_torch" in ran else [])
        for slow, fast in pairs:
            line[f"{slow}_over_{fast}"] = round(line[f"{slow}_ms"] / line[f"{fast}_ms"], 2)
            line[f"{fast}_beats_{slow}_beyond_spread"] = bool(max(times[fast]) < min(times[slow]))
        if "rgb_torch" in ran:
            line["rgb_native_psnr_all_max_abs_dev"] = float((scores["rgb_native"][0] - scores["rgb_torch"][0]).abs().max())
            line["rgb_native_ssim_mean_max_abs_dev"] = float((scores["rgb_native"][1] - scores["rgb_torch"][1]).abs().max())
        # the native launches one by one (events around each launch: a pass of its own, after the timing)
        buf = (L.ProfEntry * 64)()
        hc, wc = h - 2 * CROP, w - 2 * CROP
        for arm, samples in (("rgb_native", 3 * b * hc * wc), ("yuv_native", b * (hc * wc + 2 * (hc // 2) * (wc // 2)))):
            L.lib().resr_profile_begin()
            calls[arm]()
            torch.cuda.synchronize()
            n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), 64))
            entries = [buf[i] for i in range(n)]
            line[f"{arm}_launches"] = n
            tile_ms = sum(e.ms for e in entries if e.kernel_id == TILE_ID)
            line[f"{arm}_tile_ms"] = round(tile_ms, 4)
            line[f"{arm}_finish_ms"] = round(sum(e.ms for e in entries if e.kernel_id == FINISH_ID), 4)
            line[f"{arm}_tile_gb_per_s_of_bytes_read_once"] = round(samples * 2.0 / (tile_ms * 1e-3) / 1e9, 1)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del sr, hr, sr_yuv, hr_yuv, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
