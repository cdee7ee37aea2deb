"""What a NIQE score costs on the device: the torch path (`image_quality_assessment.NIQE`, float64 framework ops) against the native
path (`NativeNIQE`, csrc/niqe.hip) from a float batch and from a uint8 frame, and against the native path with the native tail
(`NativeNIQE(..., tail="native")`, resr_niqe_score: features -> score in two more launches, no host round trip) from a uint8 frame, on

    8k      one 7680 x 4320 image (the x4 result of a 1080p frame; 80 x 45 blocks of 96 x 96)
    16x1k   sixteen 1024 x 1024 images (10 x 10 blocks each)

of smooth colour fields plus grain (seeded).  The arms are alternated round by round in one process; a round is `--calls` calls of one
arm between two device events; the figure of an arm is the median over `--rounds` rounds, its spread their minimum and maximum.  Peak
memory is torch.cuda.max_memory_allocated over one call of the arm, above what the inputs hold.  The scores of the arms are compared
too (the native luma is one stated fp32 order: a near-tie pixel may round the other way than torch's matmul, DESIGN "Native NIQE").
A last, separate pass times the native launches one by one (resr_profile_*).  The yardstick is the torch path of the same run -- and,
for the native tail, the native-features + torch-tail arm (`native_u8`) of the same run, never the new arm itself; every figure is
recorded, whatever it is.  `forward_u8_ms` (3.26, DESIGN "uint8 frame path") is the frame the 8K call scores.

    python tools/bench_niqe.py [--rounds 5] [--calls 3] [--niqe_model_path tests/golden/niqe_model.mat] [--out profiles/niqe_tail.jsonl]
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
from real_esrgan_pytorch_amd.image_quality_assessment import NIQE, NativeNIQE  # noqa: E402

SIZES = {"8k": (1, 4320, 7680), "16x1k": (16, 1024, 1024)}
ARMS = ("torch", "native_f32", "native_u8", "native_u8_tail")
STAGES = {34000: "luma_f32", 34001: "luma_u8", 34100: "half", 34200: "mscn_scale1", 34201: "mscn_scale2", 34300: "aggd"}
TAIL_STAGES = {34400: "tail_stats", 34500: "tail_eig"}
FORWARD_U8_MS = 3.26
CROP = 4


def make_frames(b, h, w):
    """uint8 [b,h,w,3] on the device: a smooth field (bicubic from 1/8 size) plus 15 % grain, as the harness images."""
    g = torch.Generator(device="cuda").manual_seed(0)
    low = torch.rand(b, 3, h // 8, w // 8, device="cuda", generator=g)
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic").clamp_(0, 1).mul_(0.85)
    x.add_(torch.rand(b, 3, h, w, device="cuda", generator=g).mul_(0.15)).clamp_(0, 1)
    return (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


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
    ap.add_argument("--niqe_model_path", default=os.path.join(ROOT, "tests", "golden", "niqe_model.mat"))
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_niqe: needs the MI355X")
    torch.cuda.set_device(0)
    L = R._lib
    modules = {"torch": NIQE(CROP, args.niqe_model_path).cuda(), "native": NativeNIQE(CROP, args.niqe_model_path).cuda(),
               "native_tail": NativeNIQE(CROP, args.niqe_model_path, tail="native").cuda()}
    for size, (b, h, w) in SIZES.items():
        u8 = make_frames(b, h, w)
        # (divided on the host: one IEEE division per byte, the frame path's (float)byte / 255.0f; the device's division is not correctly rounded)
        f32 = (u8.permute(0, 3, 1, 2).cpu().float() / 255.0).contiguous().cuda()
        calls = {"torch": lambda: modules["torch"](f32), "native_f32": lambda: modules["native"](f32), "native_u8": lambda: modules["native"](u8),
                 "native_u8_tail": lambda: modules["native_tail"](u8)}
        line = dict(tool="bench_niqe", size=size, batch=b, height=h, width=w, crop_border=CROP, block=96, rounds=args.rounds, calls=args.calls,
                    yardstick="torch (NIQE, the same run)", device=torch.cuda.get_device_name(0),
                    arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
        scores = {}
        for arm in ARMS:                      # warm-up: code objects, tables, the allocator's pools -- and the peak of one call
            calls[arm]()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            scores[arm] = calls[arm]().double().reshape(-1).cpu()
            line[f"{arm}_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        times = {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                times[arm].append(timed(calls[arm], args.calls)[0])
        for arm in ARMS:
            line[f"{arm}_ms"] = round(statistics.median(times[arm]), 3)
            line[f"{arm}_ms_min_max"] = [round(min(times[arm]), 3), round(max(times[arm]), 3)]
        for arm in ARMS[1:]:
            line[f"torch_over_{arm}"] = round(line["torch_ms"] / line[f"{arm}_ms"], 2)
            line[f"{arm}_beats_torch_beyond_spread"] = bool(max(times[arm]) < min(times["torch"]))
            line[f"{arm}_score_max_rel_dev"] = float(((scores[arm] - scores["torch"]).abs() / scores["torch"].abs()).max())
        line["score_mean_torch"] = float(scores["torch"].mean())
        line["native_u8_equals_native_f32"] = bool(torch.equal(scores["native_u8"], scores["native_f32"]))
        # the native launches one by one (events around each launch: a pass of its own, after the timing)
        L.lib().resr_profile_begin()
        calls["native_f32"]()
        calls["native_u8"]()
        torch.cuda.synchronize()
        buf = (L.ProfEntry * 64)()
        n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), 64))
        stages = {}
        for e in (buf[i] for i in range(n)):
            if e.kernel_id in STAGES:
                stages[STAGES[e.kernel_id]] = round(e.ms, 4)
        line["native_stage_ms"] = stages
        line["native_tail_ms"] = round(line["native_u8_ms"] - sum(v for k, v in stages.items() if k != "luma_f32"), 3)   # the torch tail and the gaps
        # the native tail: its two launches, and the call against the native-features + torch-tail arm of this run
        L.lib().resr_profile_begin()
        calls["native_u8_tail"]()
        torch.cuda.synchronize()
        n = int(L.lib().resr_profile_end(C.cast(buf, C.c_void_p), 64))
        tail = {TAIL_STAGES[e.kernel_id]: round(e.ms, 4) for e in (buf[i] for i in range(n)) if e.kernel_id in TAIL_STAGES}
        line["native_tail_stage_ms"] = tail
        line["native_tail_kernels_ms"] = round(sum(tail.values()), 4)
        line["native_tail_launches"] = n
        line["tail_yardstick"] = "native_u8 (native features + torch tail, the same run)"
        line["native_u8_over_native_u8_tail"] = round(line["native_u8_ms"] / line["native_u8_tail_ms"], 2)
        line["native_u8_tail_beats_native_u8_beyond_spread"] = bool(max(times["native_u8_tail"]) < min(times["native_u8"]))
        line["native_u8_tail_vs_native_u8_score_max_rel_dev"] = float(((scores["native_u8_tail"] - scores["native_u8"]).abs() / scores["native_u8"].abs()).max())
        line["forward_u8_ms"] = FORWARD_U8_MS
        line["native_u8_over_forward_u8"] = round(line["native_u8_ms"] / FORWARD_U8_MS, 3)
        line["native_u8_tail_over_forward_u8"] = round(line["native_u8_tail_ms"] / FORWARD_U8_MS, 3)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del u8, f32, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
