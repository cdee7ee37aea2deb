"""What it costs to let a finished frame leave the device as a PNG file (png_encode.encode_png, csrc/png_encode.hip), in three parts:

  kernel   a photo-like 7680x4320 and 3840x2160 frame (bench_jpeg_encode.photo_like) and an anime-like flat 7680x4320 frame: the device
           encode (HIP events around the four launches; the launches one by one through resr_profile_*), next to `forward_u8` of a
           1920x1080 frame and the device JPEG encode (quality 95, 4:2:0) timed in the same rounds, and the host's arms on the same
           frames and rounds by wall clock: `Image.save` as PNG at compress level 6 (what inference_frames does with --ext same) and at
           level 1.  File sizes: ours against Pillow's.
  stream   FrameStream(depth=2) host to host at 1080p -> x4: copy=True, copy=False, with `jpeg` set and with `png` set, frames/s.
  folder   inference_frames end to end on a folder of 1080p PNGs: --ext same / jpg / png, each with --decode_workers 8, frames/s.

The arms of a part are alternated round by round in one process; a figure is the median over `--rounds` rounds with its minimum and
maximum.  Every figure is recorded, whatever it is.

    python tools/bench_png_encode.py [--parts kernel,stream,folder] [--rounds 5] [--frames 24] [--files 4] [--folder_rounds 3] [--out profiles/png_encode.jsonl]
"""
import argparse
import ctypes as C
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from bench_jpeg_encode import QUALITY, device_ms, emit, model_1080p, photo_like, summary, wall_ms  # noqa: E402

KERNEL_IDS = {35300: "filter", 35400: "segment", 35500: "scan", 35600: "copy"}


def anime_like(h, w, seed=0):
    """uint8 [1,h,w,3] on the device: a few hundred flat rectangles with 0.5 % speckle."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.zeros(h, w, 3, dtype=torch.uint8, device="cuda")
    x[:] = torch.tensor([200, 180, 150], dtype=torch.uint8, device="cuda")
    for _ in range(300):
        y0, x0 = int(torch.randint(0, h, (1,), generator=g, device="cuda")), int(torch.randint(0, w, (1,), generator=g, device="cuda"))
        hh, ww = int(torch.randint(16, h // 4, (1,), generator=g, device="cuda")), int(torch.randint(16, w // 4, (1,), generator=g, device="cuda"))
        x[y0:y0 + hh, x0:x0 + ww] = torch.randint(0, 256, (3,), generator=g, device="cuda").to(torch.uint8)
    hits = torch.rand(h, w, device="cuda", generator=g) < 0.005
    x[hits] = torch.randint(0, 256, (int(hits.sum()), 3), generator=g, device="cuda").to(torch.uint8)
    return x[None].contiguous()


def head():
    return dict(tool="bench_png_encode", device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
                segment_bytes=R._lib.RESR_PNG_DEFAULT_SEGMENT_BYTES)


def part_kernel(args):
    L = R._lib
    model = model_1080p()
    x1080 = photo_like(1080, 1920, 1)
    for name, make in (("photo_8k", lambda: photo_like(4320, 7680)), ("photo_4k", lambda: photo_like(2160, 3840)), ("anime_8k", lambda: anime_like(4320, 7680))):
        frame = make()
        h, w = frame.shape[1:3]
        host = frame[0].cpu().numpy()
        image = Image.fromarray(host)
        sizes = {}

        def pil_png(level):
            out = io.BytesIO()
            image.save(out, "PNG", compress_level=level)
            sizes[level] = out.tell()
        arms = {"device_encode_ms": lambda: device_ms(lambda: R.encode_png(frame)),
                "device_jpeg_encode_ms": lambda: device_ms(lambda: R.encode_jpeg(frame, QUALITY, "420")),
                "forward_u8_1080p_ms": lambda: device_ms(lambda: model.forward_u8(x1080)),
                "pil_png_level6_ms": lambda: wall_ms(lambda: pil_png(6)),
                "pil_png_level1_ms": lambda: wall_ms(lambda: pil_png(1))}
        buf, lengths = R.encode_png(frame)          # warm-up: code objects, the workspace, the allocator's pools
        R.encode_jpeg(frame, QUALITY, "420")
        model.forward_u8(x1080)
        torch.cuda.synchronize()
        size_bytes = int(lengths.item())
        decoded = np.asarray(Image.open(io.BytesIO(buf[0, :size_bytes].cpu().numpy().tobytes())))
        line = dict(head(), part="kernel", frame=name, height=h, width=w, rounds=args.rounds, raw_bytes=h * w * 3, file_bytes=size_bytes,
                    pillow_decodes_it_to_the_frame=bool(np.array_equal(decoded, host)), max_bytes=R.png_max_bytes(frame.shape),
                    workspace_bytes=int(L.lib().resr_png_encode_workspace_bytes(C.byref(L.PngEncDesc(1, h, w, 3, 8, 0)))))
        del buf, decoded
        times = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm, fn in arms.items():
                times[arm].append(fn())
        for arm in arms:
            summary(line, arm, times[arm])
        line["pillow_level6_file_bytes"], line["pillow_level1_file_bytes"] = sizes[6], sizes[1]
        line["file_over_pillow_level6"] = round(size_bytes / sizes[6], 4)
        line["pil_level6_over_device_encode"] = round(line["pil_png_level6_ms"] / line["device_encode_ms"], 1)
        line["pil_level1_over_device_encode"] = round(line["pil_png_level1_ms"] / line["device_encode_ms"], 1)
        line["encode_over_forward_u8"] = round(line["device_encode_ms"] / line["forward_u8_1080p_ms"], 3)
        entries = (L.ProfEntry * 16)()          # the launches one by one (events around each launch: a pass of its own, after the timing)
        L.lib().resr_profile_begin()
        R.encode_png(frame)
        torch.cuda.synchronize()
        for e in list(entries)[:int(L.lib().resr_profile_end(C.cast(entries, C.c_void_p), 16))]:
            if e.kernel_id in KERNEL_IDS:
                line[f"{KERNEL_IDS[e.kernel_id]}_kernel_ms"] = round(e.ms, 4)
        emit(line, args.out)
        del frame
        torch.cuda.empty_cache()


def part_stream(args):
    model = model_1080p()
    frames = [photo_like(1080, 1920, s)[0].cpu().numpy() for s in range(4)]
    feed = [frames[i % 4] for i in range(args.frames)]
    streams = {name: (R.FrameStream(model, depth=2), name == "copy") for name in ("copy", "view", "jpeg", "png")}
    streams["jpeg"][0].jpeg = dict(quality=QUALITY, subsampling="420")
    streams["png"][0].png = {}

    def run(name):
        fs, copy = streams[name]
        t, total = time.perf_counter(), 0
        for out in fs.map(feed, copy=copy):
            total += out.size
        return args.frames / (time.perf_counter() - t), total / args.frames
    line = dict(head(), part="stream", frame="1920x1080 photo-like -> x4", depth=2, frames_per_round=args.frames, rounds=args.rounds)
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
    line["png_fallbacks"] = streams["png"][0].png_fallbacks
    line["png_over_view"] = round(line["png_frames_per_s"] / line["view_frames_per_s"], 3)
    line["png_over_jpeg"] = round(line["png_frames_per_s"] / line["jpeg_frames_per_s"], 3)
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
        arms = ("same", "jpg", "png")

        def run(ext):
            out = os.path.join(tmp, "sr_" + ext)
            a = inference_frames.get_parser().parse_args(["--inputs_dir", os.path.join(tmp, "lr"), "--output_dir", out, "--weights_path", os.path.join(tmp, "w.pth"),
                                                          "--model_type", "compact", "--precision", "fast", "--ext", ext, "--decode_workers", "8",
                                                          "--jpeg_quality", str(QUALITY)])
            stdout, sys.stdout = sys.stdout, io.StringIO()
            try:
                t = time.perf_counter()
                inference_frames.main(a)
                dt = time.perf_counter() - t
            finally:
                sys.stdout = stdout
            return args.files / dt, sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) / args.files
        line = dict(head(), part="folder", frame="1920x1080 photo-like PNG -> x4", files=args.files, rounds=args.folder_rounds, decode_workers=8,
                    note="each run includes building the model and loading the checkpoint, as a user's run does")
        rates = {ext: [] for ext in arms}
        for _ in range(args.folder_rounds):
            for ext in arms:
                fps, per_file = run(ext)
                rates[ext].append(fps)
                line[f"{ext}_bytes_per_file"] = int(per_file)
        for ext in arms:
            summary(line, f"{ext}_frames_per_s", rates[ext], 2)
        line["png_over_same"] = round(line["png_frames_per_s"] / line["same_frames_per_s"], 1)
        same = np.asarray(Image.open(os.path.join(tmp, "sr_same", "f000.png")))
        line["png_file_decodes_to_the_same_frame"] = bool(np.array_equal(np.asarray(Image.open(os.path.join(tmp, "sr_png", "f000.png"))), same))
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
        sys.exit("bench_png_encode: needs the MI355X")
    torch.cuda.set_device(0)
    for part in args.parts.split(","):
        {"kernel": part_kernel, "stream": part_stream, "folder": part_folder}[part](args)


if __name__ == "__main__":
    main()
