"""Throughput of the compact generator (SRVGGNetCompact, upstream's realesr-animevideov3 / realesr-general-x4v3 shapes):
1920x1080 -> x4 frames, num_conv 16 and 32, `fast` and `exact16`, eager calls and hipGraph replays (through TiledGenerator,
halo = the receptive-field radius; a 1080p frame is one window).  One JSON line per case:
frames/s, TFLOP/s and the fraction of the MI355X's nominal dense f16 peak.

    python tools/bench_compact.py [--steps 20] [--warmup 5] [--out file.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd.tiling import TiledGenerator  # noqa: E402

F16_DENSE_PEAK = 2516.6e12   # MI355X nominal dense f16 matrix throughput, FLOP/s
H, W, S = 1080, 1920, 4


def flop_per_frame(num_conv):
    """Multiply-adds x 2 of the real channels: conv 3->64, num_conv x 64->64, conv 64->48, all at 1920x1080."""
    return 2.0 * 9 * H * W * (3 * 64 + num_conv * 64 * 64 + 64 * 3 * S * S)


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    frame = torch.rand(1, 3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    lines = []
    for num_conv in (16, 32):
        for precision in ("fast", "exact16"):
            torch.manual_seed(0)
            model = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
            tg = TiledGenerator(model, tile=None, halo=model.receptive_radius, use_graph=True)
            out = torch.empty(1, 3, H * S, W * S, device="cuda")
            for mode, fn in (("eager", lambda: model(frame)), ("hipgraph", lambda: tg(frame, out=out))):
                with torch.no_grad():
                    ms = time_ms(fn, args.steps, args.warmup)
                tflops = flop_per_frame(num_conv) / (ms * 1e-3) / 1e12
                line = dict(tool="bench_compact", num_conv=num_conv, precision=precision, mode=mode, frame=f"{W}x{H}->x{S}",
                            ms_per_frame=round(ms, 3), frames_per_s=round(1e3 / ms, 1), tflops=round(tflops, 1),
                            peak_fraction=round(tflops * 1e12 / F16_DENSE_PEAK, 3), steps=args.steps, warmup=args.warmup, **box)
                print(json.dumps(line), flush=True)
                lines.append(line)
            del model, tg
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
