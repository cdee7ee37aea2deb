"""What it costs to let a finished frame leave the device as a JPEG file (jpeg_encode.encode_jpeg, csrc/jpeg_encode.hip), in three parts:

  kernel   one 7680x4320 and one 3840x2160 frame (a smooth colour field plus grain: photo-like, not noise), quality 95, 4:2:0 and 4:4:4:
           the device encode (HIP events around the three launches; the launches one by one through resr_profile_*), next to
           `forward_u8` of a 1920x1080 frame (SRVGGNetCompact, 16 convs, x4, fast) timed in the same rounds, and the host's arms on the
           same frames and rounds by wall clock: Pillow JPEG on one thread, Pillow JPEG on a pool of 16 threads (16 encodes, time per
           frame), and `Image.save` as PNG (what inference_frames does without --ext jpg).
  stream   FrameStream(depth=2) host to host at 1080p -> x4: copy=True, copy=False and with `jpeg` set, frames/s.
  folder   inference_frames end to end on a folder of 1080p PNGs: --ext same against --ext jpg, each with --decode_workers 0 and 8, frames/s.

The arms of a part are alternated round by round in one process; a figure is the median over `--rounds` rounds with its minimum and
maximum.  Every figure is recorded, whatever it is.

    python tools/bench_jpeg_encode.py [--parts kernel,stream,folder] [--rounds 5] [--frames 24] [--files 4] [--folder_rounds 3] [--out profiles/jpeg_encode.jsonl]
"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402

SIZES = {"8k": (4320, 7680), "4k": (2160, 3840)}
QUALITY = 95
PILLOW_SUB = {"420": 2, "444": 0}
KERNEL_IDS = {35000: "segment", 35001: "segment", 35100: "scan", 35200: "copy"}


def photo_like(h, w, seed=0):
    """uint8 [1,h,w,3] on the device: a smooth field (bicubic from 1/8 size) plus 15 % grain."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    low = torch.rand(1, 3, h // 8, w // 8, device="cuda", generator=g)
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic").clamp_(0, 1).mul_(0.85)
    x.add_(torch.rand(1, 3, h, w, device="cuda", generator=g).mul_(0.15)).clamp_(0, 1)
    return (x * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def summary(line, name, values, digits=3):
    line[name] = round(statistics.median(values), digits)
    line[name + "_min_max"] = [round(min(values), digits), round(max(values), digits)]


def emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def head():
    return dict(tool="bench_jpeg_encode", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
                quality=QUALITY, restart_interval=R._lib.RESR_JPEG_DEFAULT_INTERVAL)


def model_1080p():
    torch.manual_seed(0)
    return R.SRVGGNetCompact(num_conv=16, upscale=4, precision="fast").cuda().eval().requires_grad_(False)


def part_kernel(args):
    L = R._lib
    model = model_1080p()
    x1080 = photo_like(1080, 1920, 1)
    pool = ThreadPoolExecutor(max_workers=16)
    for size, (h, w) in SIZES.items():
        frame = photo_like(h, w)
        host = frame[0].cpu().numpy()
        images = [Image.fromarray(host) for _ in range(16)]          # one Image object per pool thread: save() keeps its options on the object
        image = images[0]
        for sub in ("420", "444"):
            def pillow_jpeg(k=0):
                out = io.BytesIO()
                images[k].save(out, "JPEG", quality=QUALITY, subsampling=PILLOW_SUB[sub])
                return out.tell()
            arms = {"device_encode_ms": lambda: device_ms(lambda: R.encode_jpeg(frame, QUALITY, sub)),
                    "forward_u8_1080p_ms": lambda: device_ms(lambda: model.forward_u8(x1080)),
                    "pillow_jpeg_1_thread_ms": lambda: wall_ms(pillow_jpeg),
                    "pillow_jpeg_pool16_ms_per_frame": lambda: wall_ms(lambda: list(pool.map(pillow_jpeg, range(16)))) / 16}
            if sub == "420":          # (the PNG arm does not depend on the subsampling: once per size)
                arms["pil_png_save_ms"] = lambda: wall_ms(lambda: image.save(io.BytesIO(), "PNG"))
            buf, lengths = R.encode_jpeg(frame, QUALITY, sub)          # warm-up: code objects, the workspace, the allocator's pools
            model.forward_u8(x1080)
            torch.cuda.synchronize()
            size_bytes = int(lengths.item())
            opened = Image.open(io.BytesIO(buf[0, :size_bytes].cpu().numpy().tobytes()))
            decoded = np.asarray(opened).astype(np.float64)
            line = dict(head(), part="kernel", size=size, height=h, width=w, subsampling=sub, rounds=args.rounds, raw_bytes=h * w * 3, file_bytes=size_bytes,
                        pillow_file_bytes=pillow_jpeg(), psnr_of_pillows_decode_db=round(float(10 * np.log10(65025 / np.mean((decoded - host) ** 2))), 3),
                        workspace_bytes=int(L.lib().resr_jpeg_encode_workspace_bytes(C.byref(L.JpegEncDesc(1, h, w, R.jpeg_encode.JPEG_SUBSAMPLINGS[sub], QUALITY, 0)))))
            times = {arm: [] for arm in arms}
            for _ in range(args.rounds):
                for arm, fn in arms.items():
                    times[arm].append(fn())
            for arm in arms:
                summary(line, arm, times[arm])
            line["encode_over_forward_u8"] = round(line["device_encode_ms"] / line["forward_u8_1080p_ms"], 3)
            # the launches one by one (events around each launch: a pass of its own, after the timing)
            entries = (L.ProfEntry * 16)()
            L.lib().resr_profile_begin()
            R.encode_jpeg(frame, QUALITY, sub)
            torch.cuda.synchronize()
            for e in list(entries)[:int(L.lib().resr_profile_end(C.cast(entries, C.c_void_p), 16))]:
                if e.kernel_id in KERNEL_IDS:
                    line[f"{KERNEL_IDS[e.kernel_id]}_kernel_ms"] = round(e.ms, 4)
            # bytes: the segment kernel reads the frame once and writes the stuffed scan; the copy kernel reads and writes the scan once more
            scan = size_bytes - L.RESR_JPEG_HEADER_BYTES
            line["segment_kernel_bytes_read_written"] = [h * w * 3, scan]
            line["copy_kernel_bytes_read_written"] = [scan, size_bytes]
            if "segment_kernel_ms" in line:
                line["segment_kernel_gb_per_s_of_frame_read"] = round(h * w * 3 / (line["segment_kernel_ms"] * 1e-3) / 1e9, 1)
                line["segment_kernel_mpixel_per_s"] = round(h * w / (line["segment_kernel_ms"] * 1e-3) / 1e6, 1)
            emit(line, args.out)
        del frame
        torch.cuda.empty_cache()


def part_stream(args):
    model = model_1080p()
    frames = [photo_like(1080, 1920, s)[0].cpu().numpy() for s in range(4)]
    feed = [frames[i % 4] for i in range(args.frames)]
    streams = {"copy": (R.FrameStream(model, depth=2), True), "view": (R.FrameStream(model, depth=2), False),
               "jpeg": (R.FrameStream(model, depth=2), False)}
    streams["jpeg"][0].jpeg = dict(quality=QUALITY, subsampling="420")

    def run(name):
        fs, copy = streams[name]
        t, total = time.perf_counter(), 0
        for out in fs.map(feed, copy=copy):
            total += out.size
        return args.frames / (time.perf_counter() - t), total / args.frames
    line = dict(head(), part="stream", frame="1920x1080 -> x4", depth=2, frames_per_round=args.frames, rounds=args.rounds, subsampling="420")
    for name in streams:
        run(name)          # warm-up: slots, code objects
    rates = {name: [] for name in streams}
    for _ in range(args.rounds):
        for name in streams:
            fps, per_frame = run(name)
            rates[name].append(fps)
            line[f"{name}_bytes_to_host_per_frame"] = int(per_frame)
    for name in streams:
        summary(line, f"{name}_frames_per_s", rates[name], 2)
    line["jpeg_fallbacks"] = streams["jpeg"][0].jpeg_fallbacks
    line["jpeg_over_view"] = round(line["jpeg_frames_per_s"] / line["view_frames_per_s"], 3)
    for fs, _ in streams.values():
        fs.close()
    emit(line, args.out)


def part_folder(args):
    from real_esrgan_pytorch_amd import inference_frames
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "lr"))
        for i in range(args.files):
            Image.fromarray(photo_like(1080, 1920, i)[0].cpu().numpy()).save(os.path.join(tmp, "lr", f"f{i:03d}.png"))
        torch.manual_seed(0)
        torch.save({"params": R.SRVGGNetCompact(num_conv=16, upscale=4).state_dict()}, os.path.join(tmp, "w.pth"))
        arms = {f"{ext}_workers{k}": dict(ext=ext, decode_workers=k) for ext in ("same", "jpg") for k in (0, 8)}

        def run(name):
            out = os.path.join(tmp, "sr_" + name)
            a = inference_frames.get_parser().parse_args(["--inputs_dir", os.path.join(tmp, "lr"), "--output_dir", out, "--weights_path", os.path.join(tmp, "w.pth"),
                                                          "--model_type", "compact", "--precision", "fast", "--ext", arms[name]["ext"],
                                                          "--decode_workers", str(arms[name]["decode_workers"]), "--jpeg_quality", str(QUALITY)])
            stdout, sys.stdout = sys.stdout, io.StringIO()
            try:
                t = time.perf_counter()
                inference_frames.main(a)
                dt = time.perf_counter() - t
            finally:
                sys.stdout = stdout
            return args.files / dt, sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) / args.files
        line = dict(head(), part="folder", frame="1920x1080 PNG -> x4", files=args.files, rounds=args.folder_rounds, subsampling="420",
                    note="each run includes building the model and loading the checkpoint, as a user's run does")
        # what one stage costs on its own, per file, on one thread: the bound of the in-line arms
        name0 = os.path.join(tmp, "lr", "f000.png")
        line["decode_1080p_png_ms"] = round(statistics.median(wall_ms(lambda: np.asarray(Image.open(name0).convert("RGB"))) for _ in range(3)), 1)
        rates = {name: [] for name in arms}
        for _ in range(args.folder_rounds):
            for name in arms:
                fps, per_file = run(name)
                rates[name].append(fps)
                line[f"{name}_bytes_per_file"] = int(per_file)
        for name in arms:
            summary(line, f"{name}_frames_per_s", rates[name], 2)
        emit(line, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,stream,folder")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=24, help="stream: frames per round")
    ap.add_argument("--files", type=int, default=4, help="folder: files in the folder")
    ap.add_argument("--folder_rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_jpeg_encode: needs the MI355X")
    torch.cuda.set_device(0)
    for part in args.parts.split(","):
        {"kernel": part_kernel, "stream": part_stream, "folder": part_folder}[part](args)


if __name__ == "__main__":
    main()
