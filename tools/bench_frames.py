"""Host-to-host throughput of the uint8 frame path against the single-image float flow, 1920x1080 -> x4 with the compact
generator (num_conv 16 and 32, `fast` and `exact16`): a host uint8 HxWx3 array in, a host uint8 array out.

Paths, run ALTERNATING (A, B1, B2/2, B2/3, A, ...) for `--rounds` rounds in one process, so that drift of the box hits all alike:
  A      what inference.py does per image: astype(float32) / 255 -> image_to_tensor -> .to(device) -> model -> clamp_ -> tensor_to_image
  B1     upscale_u8 one frame at a time, plain .cuda() / .cpu()
  B2/d   FrameStream(depth=d).map, d = 2 and 3 (copy=True: the caller owns every result), and d = 2 with copy=False
  dev    device only, HIP events: model(frame fp32) against model.forward_u8(frame uint8), alternated too
Wall clock around a loop of frames that ends with every result on the host, after a warm-up of each path.  One JSON line per
(case, path): the per-round ms per frame, their median and spread (max - min), frames/s, bytes moved each way, the device name;
one `summary` line per case with the ratios and whether each exceeds the spread of the alternated repeats.

    python tools/bench_frames.py [--rounds 3] [--frames 6] [--out profiles/frames_bench_1080p.jsonl]

`--outscale O` measures the outscale path instead (frames.py, OUTSCALE), alternated the same way, per case:
  dev/forward_u8            the x4 call (untouched by outscale: the parent's launches)
  dev/forward_u8_outscale   model.forward_u8(frame, outscale=O): the fused tail (resr_compact_forward_u8_scaled)
  dev/unfused_outscale      model(frame fp32) -> resr_image_resize with uint8 output: the same result without the fusion
  B2/2, B2/2/view           FrameStream(depth=2) at x4, copy=True / copy=False
  B2/2/outscale, .../view   FrameStream(depth=2, outscale=O), copy=True / copy=False

    python tools/bench_frames.py --outscale 2 --out profiles/frames_outscale_1080p.jsonl

`--pix_fmt i420 [nv12]` measures the YUV 4:2:0 path (frames.py, YUV 4:2:0) against the rgb24 one of the same run, alternated the same
way, per case (with `--outscale O` every path below runs at that final factor, the YUV ones as the composition over the generic launches):
  dev/forward_u8            model.forward_u8(frame uint8 RGB)                  (upscale_u8(..., outscale=O) with --outscale)
  dev/forward_<fmt>         model.forward_yuv420(frame, layout=<fmt>)          (upscale_yuv420(..., outscale=O) with --outscale)
  B2/2, B2/2/view           FrameStream(depth=2), rgb24, copy=True / copy=False
  B2/2/<fmt>, .../view      FrameStream(depth=2, pix_fmt=<fmt>), copy=True / copy=False

    python tools/bench_frames.py --pix_fmt i420 nv12 --out profiles/frames_yuv420_1080p.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd import imgproc  # noqa: E402

H, W, S = 1080, 1920, 4
IN_U8, OUT_U8 = H * W * 3, H * S * W * S * 3


def path_a(model, frame):
    lr = frame.astype(np.float32) / 255.0
    t = imgproc.image_to_tensor(lr, False, False).unsqueeze_(0)
    t = t.to(device="cuda", memory_format=torch.channels_last, non_blocking=True)
    with torch.no_grad():
        sr = model(t)
    return imgproc.tensor_to_image(sr.clamp_(0, 1), False, False)


def path_b1(model, frame):
    return R.upscale_u8(model, torch.from_numpy(frame)[None].cuda())[0].cpu().numpy()


def wall_ms(run, frames):
    """ms per frame of `run(frames)`, which returns with every result on the host."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = run(frames)
    torch.cuda.synchronize()
    assert n == len(frames)
    return (time.perf_counter() - t0) * 1e3 / len(frames)


def device_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def main_outscale(args):
    o = args.outscale
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    rs = np.random.RandomState(0)
    pool = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(4)]
    many = [pool[i % 4] for i in range(args.frames * 4)]
    oh, ow = R.output_size(H, W, S, o)
    lines = []
    for num_conv in (16, 32):
        for precision in ("fast", "exact16"):
            torch.manual_seed(0)
            model = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
            x4, scaled = R.FrameStream(model, depth=2), R.FrameStream(model, depth=2, outscale=o)
            x_u8 = torch.from_numpy(pool[0])[None].cuda()
            x_f32 = R.from_u8(x_u8)
            plan = imgproc.ResizePlan(H * S, W * S, o / S, x_u8.device)
            dev = {"dev/forward_u8": lambda: model.forward_u8(x_u8),
                   "dev/forward_u8_outscale": lambda: model.forward_u8(x_u8, outscale=o, plan=plan),
                   "dev/unfused_outscale": lambda: imgproc.resize_with_plan(model(x_f32), plan, u8=True)}
            paths = {"B2/2": (lambda fr: sum(1 for _ in x4.map(fr)), OUT_U8),
                     "B2/2/view": (lambda fr: sum(1 for _ in x4.map(fr, copy=False)), OUT_U8),
                     "B2/2/outscale": (lambda fr: sum(1 for _ in scaled.map(fr)), oh * ow * 3),
                     "B2/2/outscale/view": (lambda fr: sum(1 for _ in scaled.map(fr, copy=False)), oh * ow * 3)}
            with torch.no_grad():
                same = bool(torch.equal(dev["dev/forward_u8_outscale"](), dev["dev/unfused_outscale"]()))
                for fn in dev.values():
                    for _ in range(3):
                        fn()
            for run, _ in paths.values():
                run(many[:2])
            ms = {name: [] for name in list(dev) + list(paths)}
            for _ in range(args.rounds):
                with torch.no_grad():
                    for name, fn in dev.items():
                        ms[name].append(device_ms(fn, args.device_steps))
                for name, (run, _) in paths.items():
                    ms[name].append(wall_ms(run, many))
            case = dict(tool="bench_frames", outscale=o, num_conv=num_conv, precision=precision, frame=f"{W}x{H}->{ow}x{oh}", **box)
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, v in ms.items():
                extra = dict(d2h_bytes_per_frame=paths[name][1]) if name in paths else dict(steps=args.device_steps)
                line = dict(case, path=name, ms_per_frame_rounds=[round(x, 3) for x in v], ms_per_frame=round(med[name], 3),
                            spread_ms=round(max(v) - min(v), 3), frames_per_s=round(1e3 / med[name], 2), **extra)
                print(json.dumps(line), flush=True)
                lines.append(line)
            line = dict(case, path="summary", fused_equals_unfused=same,
                        fused_over_x4_device=round(med["dev/forward_u8_outscale"] / med["dev/forward_u8"], 3),
                        fused_over_unfused_device=round(med["dev/forward_u8_outscale"] / med["dev/unfused_outscale"], 3),
                        stream_outscale_over_x4_frames_per_s=round(med["B2/2"] / med["B2/2/outscale"], 2),
                        stream_view_outscale_over_x4_frames_per_s=round(med["B2/2/view"] / med["B2/2/outscale/view"], 2))
            print(json.dumps(line), flush=True)
            lines.append(line)
            x4.close()
            scaled.close()
            del model, x4, scaled, dev, paths
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main_yuv(args):
    o = args.outscale
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    rs = np.random.RandomState(0)
    pool = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(4)]
    many = [pool[i % 4] for i in range(args.frames * 4)]
    # the same pictures as 4:2:0 frames, so that every path upscales the same content
    yuv = {fmt: [R.rgb_to_yuv420_np(f, fmt) for f in pool] for fmt in args.pix_fmt}
    many_yuv = {fmt: [yuv[fmt][i % 4] for i in range(args.frames * 4)] for fmt in args.pix_fmt}
    oh, ow = R.output_size(H, W, S, o)
    lines = []
    for num_conv in (16, 32):
        for precision in ("fast", "exact16"):
            torch.manual_seed(0)
            model = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
            streams = {"rgb24": R.FrameStream(model, depth=2, outscale=o)}
            x_u8 = torch.from_numpy(pool[0])[None].cuda()
            dev = {"dev/forward_u8": lambda: R.upscale_u8(model, x_u8, outscale=o)}
            paths = {"B2/2": (many, lambda fr: sum(1 for _ in streams["rgb24"].map(fr)), H * W * 3, oh * ow * 3),
                     "B2/2/view": (many, lambda fr: sum(1 for _ in streams["rgb24"].map(fr, copy=False)), H * W * 3, oh * ow * 3)}
            same = {}
            for fmt in args.pix_fmt:
                streams[fmt] = R.FrameStream(model, depth=2, outscale=o, pix_fmt=fmt)
                x_yuv = torch.from_numpy(yuv[fmt][0])[None].cuda()
                dev[f"dev/forward_{fmt}"] = lambda x=x_yuv, fmt=fmt: R.upscale_yuv420(model, x, fmt, outscale=o)
                paths[f"B2/2/{fmt}"] = (many_yuv[fmt], lambda fr, fmt=fmt: sum(1 for _ in streams[fmt].map(fr)), H * W * 3 // 2, oh * ow * 3 // 2)
                paths[f"B2/2/{fmt}/view"] = (many_yuv[fmt], lambda fr, fmt=fmt: sum(1 for _ in streams[fmt].map(fr, copy=False)),
                                             H * W * 3 // 2, oh * ow * 3 // 2)
                # the definition, on a timed frame: the stream's result is the composition over the RGB path
                want = R.rgb_to_yuv420(R.upscale_u8(model, R.yuv420_to_rgb(x_yuv, fmt), outscale=o), fmt)[0].cpu().numpy()
                same[fmt] = bool(np.array_equal(next(iter(streams[fmt].map(yuv[fmt][:1]))), want))
            with torch.no_grad():
                for fn in dev.values():
                    for _ in range(3):
                        fn()
            for fr, run, _, _ in paths.values():
                run(fr[:2])
            ms = {name: [] for name in list(dev) + list(paths)}
            for _ in range(args.rounds):
                with torch.no_grad():
                    for name, fn in dev.items():
                        ms[name].append(device_ms(fn, args.device_steps))
                for name, (fr, run, _, _) in paths.items():
                    ms[name].append(wall_ms(run, fr))
            case = dict(tool="bench_frames", pix_fmt=list(args.pix_fmt), outscale=o, num_conv=num_conv, precision=precision,
                        frame=f"{W}x{H}->{ow}x{oh}", **box)
            med = {name: statistics.median(v) for name, v in ms.items()}
            for name, v in ms.items():
                extra = dict(steps=args.device_steps)
                if name in paths:
                    extra = dict(h2d_bytes_per_frame=paths[name][2], d2h_bytes_per_frame=paths[name][3],
                                 d2h_gb_per_s=round(paths[name][3] / (med[name] * 1e-3) / 1e9, 2))
                line = dict(case, path=name, ms_per_frame_rounds=[round(x, 3) for x in v], ms_per_frame=round(med[name], 3),
                            spread_ms=round(max(v) - min(v), 3), frames_per_s=round(1e3 / med[name], 2), **extra)
                print(json.dumps(line), flush=True)
                lines.append(line)
            line = dict(case, path="summary", yuv_equals_composition=same)
            for fmt in args.pix_fmt:
                line[f"device_{fmt}_over_u8"] = round(med[f"dev/forward_{fmt}"] / med["dev/forward_u8"], 3)
                line[f"device_{fmt}_minus_u8_ms"] = round(med[f"dev/forward_{fmt}"] - med["dev/forward_u8"], 3)
                line[f"stream_{fmt}_over_rgb24_frames_per_s"] = round(med["B2/2"] / med[f"B2/2/{fmt}"], 2)
                line[f"stream_view_{fmt}_over_rgb24_frames_per_s"] = round(med["B2/2/view"] / med[f"B2/2/{fmt}/view"], 2)
            print(json.dumps(line), flush=True)
            lines.append(line)
            for st in streams.values():
                st.close()
            del model, streams, dev, paths
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6, help="frames per timed loop of path A and B1 (the streams take 4x as many)")
    ap.add_argument("--device-steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--outscale", type=float, default=None, help="measure the outscale path at this final factor instead (see above)")
    ap.add_argument("--pix_fmt", nargs="+", default=None, choices=["i420", "nv12"],
                    help="measure the YUV 4:2:0 path in these layouts against rgb24 instead (see above; combines with --outscale)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames.py measures on the GPU"
    if args.pix_fmt:
        return main_yuv(args)
    if args.outscale is not None:
        return main_outscale(args)
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    rs = np.random.RandomState(0)
    pool = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(4)]
    few = [pool[i % 4] for i in range(args.frames)]
    many = [pool[i % 4] for i in range(args.frames * 4)]
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for num_conv in (16, 32):
        for precision in ("fast", "exact16"):
            torch.manual_seed(0)
            model = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
            streams = {d: R.FrameStream(model, depth=d) for d in (2, 3)}
            paths = {
                "A": (few, lambda fr: sum(1 for f in fr if path_a(model, f) is not None), IN_U8 * 4, OUT_U8 * 4),
                "B1": (few, lambda fr: sum(1 for f in fr if path_b1(model, f) is not None), IN_U8, OUT_U8),
                "B2/2": (many, lambda fr: sum(1 for _ in streams[2].map(fr)), IN_U8, OUT_U8),
                "B2/3": (many, lambda fr: sum(1 for _ in streams[3].map(fr)), IN_U8, OUT_U8),
                "B2/2/view": (many, lambda fr: sum(1 for _ in streams[2].map(fr, copy=False)), IN_U8, OUT_U8),
            }
            # results must not change: the two ends of the comparison give the same bytes on a timed frame
            same = bool(np.array_equal(path_a(model, pool[0]), path_b1(model, pool[0])) and
                        np.array_equal(next(iter(streams[2].map(pool[:1]))), path_b1(model, pool[0])))
            x_f32 = R.from_u8(torch.from_numpy(pool[0])[None].cuda())
            x_u8 = torch.from_numpy(pool[0])[None].cuda()
            dev = {"dev/forward": lambda: model(x_f32), "dev/forward_u8": lambda: model.forward_u8(x_u8)}
            for name, (fr, run, _, _) in paths.items():      # warm-up of every path
                run(fr[:2])
            with torch.no_grad():
                for fn in dev.values():
                    for _ in range(3):
                        fn()
            ms = {name: [] for name in list(paths) + list(dev)}
            for _ in range(args.rounds):
                for name, (fr, run, _, _) in paths.items():
                    ms[name].append(wall_ms(run, fr))
                with torch.no_grad():
                    for name, fn in dev.items():
                        ms[name].append(device_ms(fn, args.device_steps))
            case = dict(tool="bench_frames", num_conv=num_conv, precision=precision, frame=f"{W}x{H}->x{S}", **box)
            med, spread = {}, {}
            for name, v in ms.items():
                med[name], spread[name] = statistics.median(v), max(v) - min(v)
                extra = {}
                if name in paths:
                    extra = dict(frames_per_loop=len(paths[name][0]), h2d_bytes_per_frame=paths[name][2], d2h_bytes_per_frame=paths[name][3],
                                 d2h_gb_per_s=round(paths[name][3] / (med[name] * 1e-3) / 1e9, 2))
                else:
                    extra = dict(steps=args.device_steps, out_bytes_per_frame=OUT_U8 * (4 if name == "dev/forward" else 1))
                emit(dict(case, path=name, ms_per_frame_rounds=[round(x, 3) for x in v], ms_per_frame=round(med[name], 3),
                          spread_ms=round(spread[name], 3), frames_per_s=round(1e3 / med[name], 2), **extra))
            best = min(("B2/2", "B2/3"), key=lambda k: med[k])
            emit(dict(case, path="summary", outputs_equal=same,
                      speedup_b1_over_a=round(med["A"] / med["B1"], 2), speedup_b2_depth2_over_a=round(med["A"] / med["B2/2"], 2),
                      speedup_b2_depth3_over_a=round(med["A"] / med["B2/3"], 2),
                      b2_faster_than_a_beyond_spread=bool(max(ms[best]) + 0.0 < min(ms["A"])),
                      device_u8_over_float=round(med["dev/forward_u8"] / med["dev/forward"], 3),
                      device_u8_not_slower_beyond_spread=bool(med["dev/forward_u8"] <= med["dev/forward"] + max(spread["dev/forward"], spread["dev/forward_u8"]))))
            for st in streams.values():
                st.close()
            del model, streams, paths, dev
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
