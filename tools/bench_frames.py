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
way, per case (with `--outscale O` every path below runs at that final factor; the YUV ones take the fused scaled tail, and
`dev/composed_<fmt>` is the same result as the composition over the generic launches, which is what they ran before that tail existed):
  dev/forward_u8            model.forward_u8(frame uint8 RGB)                  (upscale_u8(..., outscale=O) with --outscale)
  dev/forward_<fmt>         model.forward_yuv420(frame, layout=<fmt>)          (upscale_yuv420(..., outscale=O) with --outscale)
  B2/2, B2/2/view           FrameStream(depth=2), rgb24, copy=True / copy=False
  B2/2/<fmt>, .../view      FrameStream(depth=2, pix_fmt=<fmt>), copy=True / copy=False

    python tools/bench_frames.py --pix_fmt i420 nv12 --out profiles/frames_yuv420_1080p.jsonl

`--pix_fmt i420p10 p010` (10-bit 4:2:0, uint16 frames of 3 bytes per pixel: frames.py, 10-BIT YUV 4:2:0) may be mixed with the 8-bit
names; its paths are `upscale_yuv420p10` / `FrameStream(pix_fmt=<fmt>)` and its check the composition over the generic launches.

    python tools/bench_frames.py --pix_fmt i420 i420p10 p010 --out profiles/frames_yuv420p10_1080p.jsonl

`--out_pix_fmt FMT [--out_matrix M]` adds, for every `--pix_fmt` source, the mixed path to FMT (frames.py, MIXED FRAME FORMATS) next to the
same-format paths of the source and of FMT (FMT joins the list if it is not on it):
  dev/forward_<src>_to_<FMT>      upscale_frames(frame, (src, bt601), (FMT, M)): the fused mixed call
  dev/composed_<src>_to_<FMT>     the same result as the composition over the generic launches (with --outscale)
  B2/2/<src>_to_<FMT>, .../view   FrameStream(depth=2, pix_fmt=src, out_pix_fmt=FMT, out_matrix=M)
and the summary reports `tail_ms`: the device time of the last launch of each dev/forward_* call (the tail, by the library's own
per-launch timer, median of 5 calls outside the timed rounds) and whether the mixed tail lies between the two same-format ones.

    python tools/bench_frames.py --pix_fmt nv12 --out_pix_fmt p010 --outscale 2 --out profiles/frames_mixed_outscale_1080p.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

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


def run_cases(args, build):
    """The measurement every mode shares.  `build(model)` describes a mode for one model, a SimpleNamespace of
      head, frame   the case's fields between `tool` and `num_conv`, and its `frame` text
      dev           {name: fn}: device callables, timed with HIP events under no_grad (dev_extra: {name: more fields of its line})
      paths         {name: (frames, run, fields)}: host-to-host loops, `run(frames)` returns how many results came back; `fields` go
                    on the path's line (gbps: also d2h_gb_per_s from its d2h_bytes_per_frame)
      host_first    the paths come before the device callables in the warm-up, in every round and in the output
      check         () -> what the summary reports about equal results, taken before the warm-up
      summary       (med, spread, ms, same) -> the fields of the summary line
      streams       what to close after the case
    Owns the (num_conv, precision) grid, warm-up, the alternated rounds, the lines and --out."""
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for num_conv in (16, 32):
        for precision in ("fast", "exact16"):
            torch.manual_seed(0)
            model = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, precision=precision).cuda().eval().requires_grad_(False)
            m = build(model)

            def dev_pass(ms):            # ms None: the warm-up
                with torch.no_grad():
                    for name, fn in m.dev.items():
                        if ms is None:
                            for _ in range(3):
                                fn()
                        else:
                            ms[name].append(device_ms(fn, args.device_steps))

            def host_pass(ms):
                for name, (fr, run, _) in m.paths.items():
                    if ms is None:
                        run(fr[:2])
                    else:
                        ms[name].append(wall_ms(run, fr))

            passes = (host_pass, dev_pass) if m.host_first else (dev_pass, host_pass)
            with torch.no_grad():
                same = m.check()
            for one in passes:
                one(None)
            ms = {name: [] for name in (list(m.paths) + list(m.dev) if m.host_first else list(m.dev) + list(m.paths))}
            for _ in range(args.rounds):
                for one in passes:
                    one(ms)
            case = dict(tool="bench_frames", **m.head, num_conv=num_conv, precision=precision, frame=m.frame, **box)
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            for name, v in ms.items():
                if name in m.paths:
                    extra = dict(m.paths[name][2])
                    if m.gbps:
                        extra["d2h_gb_per_s"] = round(extra["d2h_bytes_per_frame"] / (med[name] * 1e-3) / 1e9, 2)
                else:
                    extra = dict(steps=args.device_steps, **m.dev_extra.get(name, {}))
                emit(dict(case, path=name, ms_per_frame_rounds=[round(x, 3) for x in v], ms_per_frame=round(med[name], 3),
                          spread_ms=round(spread[name], 3), frames_per_s=round(1e3 / med[name], 2), **extra))
            emit(dict(case, path="summary", **m.summary(med, spread, ms, same)))
            for st in m.streams:
                st.close()
            del model, m
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def frame_pool(args):
    rs = np.random.RandomState(0)
    pool = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(4)]
    return pool, [pool[i % 4] for i in range(args.frames * 4)]


def count(results):
    return sum(1 for _ in results)


def mode_x4(args):
    pool, many = frame_pool(args)
    few = many[:args.frames]

    def build(model):
        streams = {d: R.FrameStream(model, depth=d) for d in (2, 3)}
        x_u8 = torch.from_numpy(pool[0])[None].cuda()
        x_f32 = R.from_u8(x_u8)
        f32 = dict(frames_per_loop=len(few), h2d_bytes_per_frame=IN_U8 * 4, d2h_bytes_per_frame=OUT_U8 * 4)
        u8 = dict(h2d_bytes_per_frame=IN_U8, d2h_bytes_per_frame=OUT_U8)
        one, loop = dict(frames_per_loop=len(few), **u8), dict(frames_per_loop=len(many), **u8)
        paths = {"A": (few, lambda fr: sum(1 for f in fr if path_a(model, f) is not None), f32),
                 "B1": (few, lambda fr: sum(1 for f in fr if path_b1(model, f) is not None), one),
                 "B2/2": (many, lambda fr: count(streams[2].map(fr)), loop),
                 "B2/3": (many, lambda fr: count(streams[3].map(fr)), loop),
                 "B2/2/view": (many, lambda fr: count(streams[2].map(fr, copy=False)), loop)}

        def summary(med, spread, ms, same):
            best = min(("B2/2", "B2/3"), key=lambda k: med[k])
            return dict(outputs_equal=same, speedup_b1_over_a=round(med["A"] / med["B1"], 2),
                        speedup_b2_depth2_over_a=round(med["A"] / med["B2/2"], 2), speedup_b2_depth3_over_a=round(med["A"] / med["B2/3"], 2),
                        b2_faster_than_a_beyond_spread=bool(max(ms[best]) + 0.0 < min(ms["A"])),
                        device_u8_over_float=round(med["dev/forward_u8"] / med["dev/forward"], 3),
                        device_u8_not_slower_beyond_spread=bool(med["dev/forward_u8"] <= med["dev/forward"] + max(spread["dev/forward"], spread["dev/forward_u8"])))

        return SimpleNamespace(
            head={}, frame=f"{W}x{H}->x{S}", host_first=True, gbps=True, paths=paths, streams=list(streams.values()), summary=summary,
            dev={"dev/forward": lambda: model(x_f32), "dev/forward_u8": lambda: model.forward_u8(x_u8)},
            dev_extra={"dev/forward": dict(out_bytes_per_frame=OUT_U8 * 4), "dev/forward_u8": dict(out_bytes_per_frame=OUT_U8)},
            # results must not change: the two ends of the comparison give the same bytes on a timed frame
            check=lambda: bool(np.array_equal(path_a(model, pool[0]), path_b1(model, pool[0])) and
                               np.array_equal(next(iter(streams[2].map(pool[:1]))), path_b1(model, pool[0]))))

    return build


def mode_outscale(args):
    o = args.outscale
    pool, many = frame_pool(args)
    oh, ow = R.output_size(H, W, S, o)

    def build(model):
        x4, scaled = R.FrameStream(model, depth=2), R.FrameStream(model, depth=2, outscale=o)
        x_u8 = torch.from_numpy(pool[0])[None].cuda()
        x_f32 = R.from_u8(x_u8)
        plan = imgproc.ResizePlan(H * S, W * S, o / S, x_u8.device)
        dev = {"dev/forward_u8": lambda: model.forward_u8(x_u8),
               "dev/forward_u8_outscale": lambda: model.forward_u8(x_u8, outscale=o, plan=plan),
               "dev/unfused_outscale": lambda: imgproc.resize_with_plan(model(x_f32), plan, u8=True)}
        paths = {"B2/2": (many, lambda fr: count(x4.map(fr)), dict(d2h_bytes_per_frame=OUT_U8)),
                 "B2/2/view": (many, lambda fr: count(x4.map(fr, copy=False)), dict(d2h_bytes_per_frame=OUT_U8)),
                 "B2/2/outscale": (many, lambda fr: count(scaled.map(fr)), dict(d2h_bytes_per_frame=oh * ow * 3)),
                 "B2/2/outscale/view": (many, lambda fr: count(scaled.map(fr, copy=False)), dict(d2h_bytes_per_frame=oh * ow * 3))}

        def summary(med, spread, ms, same):
            return dict(fused_equals_unfused=same,
                        fused_over_x4_device=round(med["dev/forward_u8_outscale"] / med["dev/forward_u8"], 3),
                        fused_over_unfused_device=round(med["dev/forward_u8_outscale"] / med["dev/unfused_outscale"], 3),
                        stream_outscale_over_x4_frames_per_s=round(med["B2/2"] / med["B2/2/outscale"], 2),
                        stream_view_outscale_over_x4_frames_per_s=round(med["B2/2/view"] / med["B2/2/outscale/view"], 2))

        return SimpleNamespace(head=dict(outscale=o), frame=f"{W}x{H}->{ow}x{oh}", host_first=False, gbps=False, dev=dev, dev_extra={},
                               paths=paths, streams=[x4, scaled], summary=summary,
                               check=lambda: bool(torch.equal(dev["dev/forward_u8_outscale"](), dev["dev/unfused_outscale"]())))

    return build


def tail_ms(fn, repeats=5):
    """(kernel id, ms) of the last launch of `fn()`, by the library's in-situ profiler: the median of `repeats` calls."""
    lib = R._lib.lib()
    ms, kid = [], None
    for _ in range(repeats):
        lib.resr_profile_begin()
        try:
            fn()
        finally:
            torch.cuda.synchronize()
            buf = (R._lib.ProfEntry * 4096)()
            n = int(lib.resr_profile_end(ctypes.cast(buf, ctypes.c_void_p), 4096))
        kid = buf[n - 1].kernel_id
        ms.append(buf[n - 1].ms)
    return kid, round(statistics.median(ms), 4)


def mode_yuv(args):
    o = args.outscale
    pool, many = frame_pool(args)
    dst = args.out_pix_fmt
    sources = list(args.pix_fmt)
    if dst and dst not in args.pix_fmt:
        args.pix_fmt = list(args.pix_fmt) + [dst]          # the destination's own same-format path, next to the mixed one
    dst_matrix = args.out_matrix or "bt601"
    mixed = [(a, dst) for a in sources if (a, "bt601") != (dst, dst_matrix)] if dst else []
    # the same pictures as 4:2:0 frames, so that every path upscales the same content
    ten = set(R.frames.YUV10_LAYOUTS)

    def to_yuv(f, fmt):      # (10 bits: the same picture at level * 4, so that the two depths upscale the same content)
        return R.rgb_to_yuv420p10_np(f.astype(np.uint16) * 4, fmt) if fmt in ten else R.rgb_to_yuv420_np(f, fmt)

    def upscale(model, x, fmt):
        return (R.upscale_yuv420p10 if fmt in ten else R.upscale_yuv420)(model, x, fmt, outscale=o)

    scaled = o is not None and o != S
    plans = {}

    def composed(model, x, fmt):     # the definition as launches: generic conversion, the RGB / float path, generic conversion
        if fmt in ten:
            sr = model(R.from_yuv420p10(x, fmt))
            if scaled:
                if x.device not in plans:
                    plans[x.device] = imgproc.ResizePlan(H * S, W * S, o / S, x.device)
                sr = imgproc.resize_with_plan(sr, plans[x.device])
            return R.to_yuv420p10(sr, fmt)
        return R.rgb_to_yuv420(R.upscale_u8(model, R.yuv420_to_rgb(x, fmt), outscale=o), fmt)

    def composed_mixed(model, x, a, b):     # a's generic launches in, the float path, b's out
        sr = model(R.from_yuv420p10(x, a) if a in ten else R.from_u8(R.yuv420_to_rgb(x, a)))
        if scaled and x.device not in plans:
            plans[x.device] = imgproc.ResizePlan(H * S, W * S, o / S, x.device)
        if b in ten:
            return R.to_yuv420p10(imgproc.resize_with_plan(sr, plans[x.device]) if scaled else sr, b, dst_matrix)
        return R.rgb_to_yuv420(imgproc.resize_with_plan(sr, plans[x.device], u8=True) if scaled else R.to_u8(sr), b, dst_matrix)

    yuv = {fmt: [to_yuv(f, fmt) for f in pool] for fmt in args.pix_fmt}
    many_yuv = {fmt: [yuv[fmt][i % 4] for i in range(args.frames * 4)] for fmt in args.pix_fmt}
    oh, ow = R.output_size(H, W, S, o)
    rgb_bytes = dict(h2d_bytes_per_frame=H * W * 3, d2h_bytes_per_frame=oh * ow * 3)
    yuv_bytes = {fmt: dict(h2d_bytes_per_frame=H * W * 3 // 2 * (2 if fmt in ten else 1),
                           d2h_bytes_per_frame=oh * ow * 3 // 2 * (2 if fmt in ten else 1)) for fmt in args.pix_fmt}
    mixed_bytes = {(a, b): dict(h2d_bytes_per_frame=yuv_bytes[a]["h2d_bytes_per_frame"], d2h_bytes_per_frame=yuv_bytes[b]["d2h_bytes_per_frame"])
                   for a, b in mixed}

    def build(model):
        streams = {"rgb24": R.FrameStream(model, depth=2, outscale=o)}
        x_u8 = torch.from_numpy(pool[0])[None].cuda()
        dev = {"dev/forward_u8": lambda: R.upscale_u8(model, x_u8, outscale=o)}
        paths = {"B2/2": (many, lambda fr: count(streams["rgb24"].map(fr)), rgb_bytes),
                 "B2/2/view": (many, lambda fr: count(streams["rgb24"].map(fr, copy=False)), rgb_bytes)}
        x_yuv = {}
        for fmt in args.pix_fmt:
            streams[fmt] = R.FrameStream(model, depth=2, outscale=o, pix_fmt=fmt)
            x_yuv[fmt] = torch.from_numpy(yuv[fmt][0])[None].cuda()
            dev[f"dev/forward_{fmt}"] = lambda fmt=fmt: upscale(model, x_yuv[fmt], fmt)
            if scaled:
                dev[f"dev/composed_{fmt}"] = lambda fmt=fmt: composed(model, x_yuv[fmt], fmt)
            paths[f"B2/2/{fmt}"] = (many_yuv[fmt], lambda fr, fmt=fmt: count(streams[fmt].map(fr)), yuv_bytes[fmt])
            paths[f"B2/2/{fmt}/view"] = (many_yuv[fmt], lambda fr, fmt=fmt: count(streams[fmt].map(fr, copy=False)), yuv_bytes[fmt])
        for a, b in mixed:
            key = f"{a}_to_{b}"
            streams[key] = R.FrameStream(model, depth=2, outscale=o, pix_fmt=a, out_pix_fmt=b, out_matrix=dst_matrix)
            dev[f"dev/forward_{key}"] = lambda a=a, b=b: R.upscale_frames(model, x_yuv[a], (a, "bt601"), (b, dst_matrix), outscale=o)
            if scaled:
                dev[f"dev/composed_{key}"] = lambda a=a, b=b: composed_mixed(model, x_yuv[a], a, b)
            paths[f"B2/2/{key}"] = (many_yuv[a], lambda fr, key=key: count(streams[key].map(fr)), mixed_bytes[(a, b)])
            paths[f"B2/2/{key}/view"] = (many_yuv[a], lambda fr, key=key: count(streams[key].map(fr, copy=False)), mixed_bytes[(a, b)])

        def check():     # the definition, on a timed frame: the stream's result is the composition over the RGB path
            same = {}
            for fmt in args.pix_fmt:
                want = composed(model, x_yuv[fmt], fmt)[0].cpu().numpy()
                same[fmt] = bool(np.array_equal(next(iter(streams[fmt].map(yuv[fmt][:1]))), want))
            for a, b in mixed:
                want = composed_mixed(model, x_yuv[a], a, b)[0].cpu().numpy()
                same[f"{a}_to_{b}"] = bool(np.array_equal(next(iter(streams[f"{a}_to_{b}"].map(yuv[a][:1]))), want))
            return same

        def summary(med, spread, ms, same):
            line = dict(yuv_equals_composition=same)
            for fmt in args.pix_fmt:
                line[f"device_{fmt}_over_u8"] = round(med[f"dev/forward_{fmt}"] / med["dev/forward_u8"], 3)
                line[f"device_{fmt}_minus_u8_ms"] = round(med[f"dev/forward_{fmt}"] - med["dev/forward_u8"], 3)
                line[f"stream_{fmt}_over_rgb24_frames_per_s"] = round(med["B2/2"] / med[f"B2/2/{fmt}"], 2)
                line[f"stream_view_{fmt}_over_rgb24_frames_per_s"] = round(med["B2/2/view"] / med[f"B2/2/{fmt}/view"], 2)
                if scaled:       # the fused tail against the composition of the same run
                    a, b = f"dev/forward_{fmt}", f"dev/composed_{fmt}"
                    line[f"device_{fmt}_fused_over_composed"] = round(med[a] / med[b], 3)
                    line[f"device_{fmt}_fused_minus_composed_ms"] = round(med[a] - med[b], 3)
                    line[f"device_{fmt}_fused_not_slower_beyond_spread"] = bool(med[a] <= med[b] + max(spread[a], spread[b]))
            if mixed:            # the tails alone: the mixed one reads the source's words and writes the destination's
                with torch.no_grad():
                    tails = {name[len("dev/forward_"):]: tail_ms(fn) for name, fn in dev.items() if name.startswith("dev/forward_") and name != "dev/forward_u8"}
                line["tail_ms"] = {k: dict(kernel_id=v[0], ms=v[1]) for k, v in tails.items()}
                for a, b in mixed:
                    key = f"{a}_to_{b}"
                    lo, hi = sorted((tails[a][1], tails[b][1]))
                    line[f"tail_{key}_between_same_format_tails"] = bool(lo <= tails[key][1] <= hi)
                    line[f"device_{key}_over_{a}"] = round(med[f"dev/forward_{key}"] / med[f"dev/forward_{a}"], 3)
                    line[f"device_{key}_over_{b}"] = round(med[f"dev/forward_{key}"] / med[f"dev/forward_{b}"], 3)
                    line[f"stream_{key}_over_{a}_frames_per_s"] = round(med[f"B2/2/{a}"] / med[f"B2/2/{key}"], 2)
                    line[f"stream_view_{key}_over_{a}_frames_per_s"] = round(med[f"B2/2/{a}/view"] / med[f"B2/2/{key}/view"], 2)
            return line

        return SimpleNamespace(head=dict(pix_fmt=list(args.pix_fmt), outscale=o, **(dict(out_pix_fmt=dst, out_matrix=dst_matrix) if dst else {})), frame=f"{W}x{H}->{ow}x{oh}", host_first=False, gbps=True,
                               dev=dev, dev_extra={}, paths=paths, streams=list(streams.values()), summary=summary, check=check)

    return build


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=6, help="frames per timed loop of path A and B1 (the streams take 4x as many)")
    ap.add_argument("--device-steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--outscale", type=float, default=None, help="measure the outscale path at this final factor instead (see above)")
    ap.add_argument("--pix_fmt", nargs="+", default=None, choices=["i420", "nv12", "i420p10", "p010"],
                    help="measure the YUV 4:2:0 path in these layouts (8-bit, or the 10-bit i420p10 / p010) against rgb24 instead (see above; combines with --outscale)")
    ap.add_argument("--out_pix_fmt", default=None, choices=["i420", "nv12", "i420p10", "p010"],
                    help="with --pix_fmt: also measure the mixed path from every --pix_fmt source to this format (see above)")
    ap.add_argument("--out_matrix", default=None, choices=["bt601", "bt709"], help="the matrix of --out_pix_fmt (default bt601, the sources')")
    args = ap.parse_args()
    if args.out_pix_fmt and not args.pix_fmt:
        ap.error("--out_pix_fmt needs --pix_fmt (the sources)")
    assert torch.cuda.is_available(), "bench_frames.py measures on the GPU"
    mode = mode_yuv if args.pix_fmt else mode_outscale if args.outscale is not None else mode_x4
    run_cases(args, mode(args))


if __name__ == "__main__":
    main()
