"""Device time of the image modes (frames.py, IMAGE MODES): the fused call `SRVGGNetCompact.forward_image` against the composition
`from_image -> forward -> to_image` of the same result, 1920x1080 -> x4, compact generator with 16 convs, `fast` and `exact16`, for
rgba8, rgb16 and grey8; for rgba8 also against two `forward_u8` calls (what a caller without the alpha path would run for colour
and alpha, the alpha plane already replicated to RGB and the merge into RGBA not counted).

The sides of a mode run ALTERNATING for `--rounds` rounds in one process, each timed with device events over `--steps` calls after a
warm-up, so that drift of the box hits all alike.  Before the timing the fused result is compared with the composition's on the timed
images: they must be equal.  One JSON line per (precision, mode, path): the per-round ms per call, their median and spread
(max - min), the bytes of the images in and out; one `summary` line per (precision, mode) with the ratios and whether the fused
call is faster beyond the spread of the alternated repeats.

`--outscale F` (frames.py, IMAGE MODES): the same alternation at a final factor F -- `forward_image(images, outscale=F)`, whose last
kernel resizes in LDS, against the composition `from_image -> forward -> resize_with_plan -> to_image`, which writes and re-reads the
fp32 x4 frames and the fp32 resized frames; both sides share one `imgproc.ResizePlan`.  The summary also says whether the fused call
is SLOWER beyond the spread: then `frames.upscale_image` should take the composition for that mode.

    python tools/bench_image_modes.py [--rounds 5] [--steps 10] [--out profiles/image_modes_1080p.jsonl]
    python tools/bench_image_modes.py --outscale 2 --out profiles/image_modes_outscale_1080p.jsonl
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402

H, W, S, NUM_CONV = 1080, 1920, 4, 16
MODES = {"rgba8": (4, np.uint8), "rgb16": (3, np.uint16), "grey8": (1, np.uint8)}


def device_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def sides(model, name, images, outscale=None):
    """{path: callable} of one mode, and the bytes of its images in and out."""
    channels = 1 if images.dim() == 3 else images.shape[3]
    nbytes = images.numel() * images.element_size()
    if outscale is None:
        paths = {"forward_image": lambda: model.forward_image(images),
                 "composition": lambda: R.to_image(model(R.from_image(images)), channels, images.dtype)}
        out_bytes = nbytes * S * S
        plan = None
    else:
        from real_esrgan_pytorch_amd.imgproc import ResizePlan, resize_with_plan
        plan = ResizePlan(H * S, W * S, outscale / S, images.device)
        paths = {"forward_image": lambda: model.forward_image(images, outscale=outscale, plan=plan),
                 "composition": lambda: R.to_image(resize_with_plan(model(R.from_image(images)), plan), channels, images.dtype)}
        out_bytes = plan.out_h * plan.out_w * channels * images.element_size()
    if name == "rgba8":
        colour = images[..., :3].contiguous()
        alpha = images[..., 3:].expand(-1, -1, -1, 3).contiguous()
        paths["two_forward_u8"] = lambda: (model.forward_u8(colour, outscale=outscale, plan=plan), model.forward_u8(alpha, outscale=outscale, plan=plan))
    return paths, nbytes, out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--outscale", type=float, default=None, help="final factor (default: the model's x4, no resize)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_image_modes.py measures on the GPU"
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    rs = np.random.RandomState(0)
    for precision in ("fast", "exact16"):
        torch.manual_seed(0)
        model = R.SRVGGNetCompact(num_conv=NUM_CONV, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
        for name, (channels, dtype) in MODES.items():
            top = np.iinfo(dtype).max
            shape = (1, H, W) if channels == 1 else (1, H, W, channels)
            images = torch.from_numpy(rs.randint(0, top + 1, size=shape).astype(dtype)).cuda()
            paths, in_bytes, out_bytes = sides(model, name, images, args.outscale)
            with torch.no_grad():
                fused, composed = paths["forward_image"](), paths["composition"]()
                same = bool(torch.equal(fused.view(torch.uint8), composed.view(torch.uint8)))     # results must not change
                del fused, composed
                for fn in paths.values():
                    for _ in range(3):
                        fn()
                ms = {p: [] for p in paths}
                for _ in range(args.rounds):
                    for p, fn in paths.items():
                        ms[p].append(device_ms(fn, args.steps))
            scale = S if args.outscale is None else f"{args.outscale:g}"
            case = dict(tool="bench_image_modes", mode=name, num_conv=NUM_CONV, precision=precision, frame=f"{W}x{H}->x{scale}", **box)
            med = {p: statistics.median(v) for p, v in ms.items()}
            spread = {p: max(v) - min(v) for p, v in ms.items()}
            for p, v in ms.items():
                emit(dict(case, path=p, ms_per_call_rounds=[round(x, 3) for x in v], ms_per_call=round(med[p], 3), spread_ms=round(spread[p], 3),
                          steps=args.steps, in_bytes=in_bytes, out_bytes=out_bytes))
            summary = dict(fused_equals_composition=same, fused_over_composition=round(med["forward_image"] / med["composition"], 3),
                           fused_minus_composition_ms=round(med["forward_image"] - med["composition"], 3),
                           fused_faster_beyond_spread=bool(max(ms["forward_image"]) < min(ms["composition"])),
                           fused_slower_beyond_spread=bool(min(ms["forward_image"]) > max(ms["composition"])))
            if "two_forward_u8" in paths:
                summary["fused_over_two_forward_u8"] = round(med["forward_image"] / med["two_forward_u8"], 3)
            emit(dict(case, path="summary", **summary))
            del images, paths
            torch.cuda.empty_cache()
        del model
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
