"""Directory super-resolution on the uint8 frame path (frames.py): every image of a folder, pipelined.

    python -m real_esrgan_pytorch_amd.inference_frames --inputs_dir lr/ --output_dir sr/ --weights_path g.pth \\
        [--model_type rrdb|compact --num_conv 16 --act_type prelu --precision fast|exact16|strict --depth 2 --outscale 2 --keep_mode
         --niqe --niqe_tail torch|native --reference_dir gt/ --score_channels y|rgb
         --ext same|jpg|png --jpeg_quality 95 --jpeg_subsampling 420|444 --decode_workers K]

The model is built and the checkpoint loaded exactly as `inference.py` does for one image; the files of `--inputs_dir` are then
walked in sorted order: PIL decode -> `FrameStream.map` (upload, compute and download of successive frames overlap) -> PIL
encode under the same file name in `--output_dir`.  Each written image equals what `inference.py` writes for that file on its
own.  `--outscale F` (default: the model's factor) writes `frames.output_size` images instead: the model's output resized by
F / factor with the reference's antialiased bicubic `image_resize`, on the device (frames.py, OUTSCALE).  Frames of different sizes may be mixed (a change of size drains the pipeline).  Video containers are not read here: extract
frames first (ffmpeg -i in.mp4 lr/%06d.png), as upstream's inference_realesrgan_video.py does internally.

`--keep_mode` (default off: every file is decoded with `.convert("RGB")`, as above): a file whose PIL mode is `L` (8-bit grey), `RGBA`
or `I;16` (16-bit grey) keeps it, and `LA` becomes RGBA: such a file goes through `frames.upscale_image` on its own -- alpha through the
network as a grey image, 16 bits in and 16 bits out -- and is written in the mode it came in.  RGB files, and every other mode through
`.convert("RGB")`, keep going through the pipelined `FrameStream`.  `--outscale F` applies to the kept modes too
(`upscale_image(..., outscale=F)`: frames.py, IMAGE MODES).  PIL has no 16-bit RGB or RGBA mode: those are `frames.upscale_image` on
arrays of your own.

`--niqe`: every frame of the RGB stream is scored where the last kernel wrote it -- `image_quality_assessment.niqe_native` on the uint8
device frame, on the compute stream, before the download (crop_border = the model's factor, as test.py; the prior from
`--niqe_model_path`) -- and the scores are read once, at the end: `NIQE <file>: <score>` per frame in input order, then
`NIQE mean: <score>`.  Files that `--keep_mode` takes out of the RGB stream are not scored.  `--niqe_tail native` (default `torch`)
turns the features into the score on the device too (`niqe_score_native`): a frame's score is enqueued behind its features and the
host never waits for it before the one read at the end.

`--reference_dir DIR`: every frame of the RGB stream is scored against the file of the same name in DIR, uploaded as uint8 HWC --
`image_quality_assessment.full_ref_native` (PSNR and SSIM of the Y channel, crop_border = the model's factor) on the uint8 device
frame, on the compute stream, as `--niqe` -- and the scores are read once, at the end: `PSNR/SSIM <file>: <dB> <ssim>` per frame, then
`PSNR/SSIM mean: ...`.  A missing reference, or one whose size is not the written image's (an `--outscale` that does not lead to the
reference's size), is an error that names the file, raised before any frame is computed.  `--score_channels rgb` (default `y`)
scores the three RGB channels instead -- `full_ref_channels_native`: the PSNR over all three (BasicSR's `test_y_channel: false`) and
the mean of the channels' SSIMs -- in the same lines.

`--ext jpg` (default `same`: everything above, byte for byte): every frame of the RGB stream leaves the device as a finished JPEG file
(`FrameStream.jpeg`, `jpeg_encode.encode_jpeg`: `--jpeg_quality` 1..100, `--jpeg_subsampling` 420 or 444) and is written as
`<stem>.jpg` straight from the returned bytes: the host encodes nothing and a few MB cross the bus instead of the raw frame.  `--niqe`
and `--reference_dir` still score the raw frame.  Files that `--keep_mode` takes out of the stream keep their extension and the PIL path.

`--ext png`: the lossless twin -- every frame of the RGB stream leaves the device as a finished PNG file (`FrameStream.png`,
`png_encode.encode_png`) and is written as `<stem>.png` from the returned bytes; the host's single-threaded PNG encoder, the slowest stage
of `--ext same` on large frames, is not run.  With `--keep_mode` the kept files go the same way: `upscale_image`, then `encode_png` of the
device tensor -- an `L` file becomes an 8-bit grey PNG, an `RGBA` or `LA` file an 8-bit RGBA one, an `I;16` file a 16-bit grey one.

`--decode_workers K` (default 0: the in-line decode above): the input files are decoded by a pool of min(K, 16) threads, in input
order, at most 2 K files ahead of the stream.
"""
import argparse
import os

import numpy as np
import torch

from . import config
from .compact import SRVGGNetCompact
from .frames import FrameStream, upscale_image
from .model import Generator, load_official_state_dict

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")


def build_model(args):
    """The model of `inference.main` (same constructor arguments, same checkpoint formats), in eval mode on config.device."""
    model_type = getattr(args, "model_type", "rrdb") or "rrdb"
    precision = getattr(args, "precision", None) or config.inference_precision
    if model_type == "compact":
        model = SRVGGNetCompact(config.in_channels, config.out_channels, 64, getattr(args, "num_conv", 16) or 16,
                                config.upscale_factor, getattr(args, "act_type", "prelu") or "prelu", precision=precision)
    elif model_type == "rrdb":
        model = Generator(config.in_channels, config.out_channels, config.upscale_factor, precision=precision)
    else:
        raise ValueError(f"--model_type must be 'rrdb' or 'compact', got {model_type!r}")
    model = model.to(memory_format=torch.channels_last, device=config.device)
    print("Build Real_ESRGAN model successfully.")
    checkpoint = torch.load(args.weights_path, map_location=lambda storage, loc: storage, weights_only=False)
    if isinstance(checkpoint, dict) and "state_dict" in checkpoint:
        model.load_state_dict({k.replace("model.", ""): v for k, v in checkpoint["state_dict"].items()})
    else:
        load_official_state_dict(model, checkpoint)
    print(f"Load Real_ESRGAN model weights `{args.weights_path}` successfully.")
    return model.eval()


def list_images(inputs_dir: str):
    return sorted(f for f in os.listdir(inputs_dir) if f.lower().endswith(IMAGE_EXTENSIONS))


KEPT_MODES = {"L": "L", "RGBA": "RGBA", "I;16": "I;16", "LA": "RGBA"}     # PIL mode of a file -> the mode it is upscaled and written in


def kept_mode(image):
    """The mode `--keep_mode` upscales and writes this PIL image in, or None for one that takes the RGB stream."""
    return KEPT_MODES.get(image.mode)


def upscale_kept(model, image, mode: str, outscale=None, png: bool = False):
    """One PIL image of a kept mode through `frames.upscale_image` (at `outscale`) -> the PIL image of that mode; `png`: the bytes of
    its PNG file instead, encoded on the device (`png_encode.png_files`)."""
    from PIL import Image
    array = np.array(image if image.mode == mode else image.convert(mode))      # (a copy: PIL's own buffer is read-only)
    images = torch.from_numpy(array)[None].to(next(model.parameters()).device)
    if png:
        from .png_encode import png_files
        return png_files(upscale_image(model, images, outscale=outscale))[0]
    return Image.fromarray(upscale_image(model, images, outscale=outscale)[0].cpu().numpy())


def main(args) -> None:
    from PIL import Image
    torch.cuda.set_device(config.device)
    model = build_model(args)
    names = list_images(args.inputs_dir)
    os.makedirs(args.output_dir, exist_ok=True)
    kept = {}           # --keep_mode: file name -> mode, for the files that leave the RGB stream below alone
    if getattr(args, "keep_mode", False):
        for name in names:
            with Image.open(os.path.join(args.inputs_dir, name)) as image:      # (reads the header only)
                if kept_mode(image) is not None:
                    kept[name] = kept_mode(image)
        names = [name for name in names if name not in kept]
    ext = getattr(args, "ext", None) or "same"
    if ext not in ("same", "jpg", "png"):
        raise ValueError(f"--ext must be 'same', 'jpg' or 'png', got {ext!r}")
    for name, mode in kept.items():
        with Image.open(os.path.join(args.inputs_dir, name)) as image:
            if ext == "png":                     # the device's bytes, as for the stream below
                name = os.path.splitext(name)[0] + ".png"
                with open(os.path.join(args.output_dir, name), "wb") as file:
                    file.write(upscale_kept(model, image, mode, getattr(args, "outscale", None), png=True))
            else:
                upscale_kept(model, image, mode, getattr(args, "outscale", None)).save(os.path.join(args.output_dir, name))
        print(f"SR image save to `{os.path.join(args.output_dir, name)}`")

    scores = []         # --niqe: one device scalar per frame of the stream, in input order
    niqe_model = None
    if getattr(args, "niqe", False):
        from .image_quality_assessment import NativeNIQE
        niqe_model = NativeNIQE(config.upscale_factor, getattr(args, "niqe_model_path", None) or config.niqe_model_path,
                                tail=getattr(args, "niqe_tail", None) or "torch").to(device=config.device)

    reference_dir = getattr(args, "reference_dir", None)
    references, full_scores = {}, []        # --reference_dir: file name -> uint8 [1,H,W,3] host tensor; one (psnr, ssim) device pair per frame
    if reference_dir:
        from .frames import output_size
        from .image_quality_assessment import full_ref_channels_native, full_ref_native
        if (getattr(args, "score_channels", None) or "y") not in ("y", "rgb"):
            raise ValueError(f"--score_channels must be 'y' or 'rgb', got {args.score_channels!r}")
        if (getattr(args, "score_channels", None) or "y") == "rgb":
            def score(frame, hr):
                r = full_ref_channels_native(frame, hr, config.upscale_factor)
                return r.psnr_all, r.ssim_mean
        else:
            def score(frame, hr):
                return full_ref_native(frame, hr, config.upscale_factor)
        for name in names:
            path = os.path.join(reference_dir, name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"--reference_dir: no reference `{path}` for `{name}`")
            with Image.open(os.path.join(args.inputs_dir, name)) as image:
                want = output_size(image.height, image.width, config.upscale_factor, getattr(args, "outscale", None))
            with Image.open(path) as image:
                if (image.height, image.width) != tuple(want):
                    raise ValueError(f"--reference_dir: the reference `{path}` is {image.height}x{image.width}, the output for `{name}` "
                                     f"{want[0]}x{want[1]} (--outscale must lead to the reference's size)")
                references[name] = torch.from_numpy(np.array(image.convert("RGB")))[None]
    pending = iter(names)                   # on_device sees the frames in input order

    def decode_one(name):
        return np.asarray(Image.open(os.path.join(args.inputs_dir, name)).convert("RGB"))

    workers = min(int(getattr(args, "decode_workers", 0) or 0), 16)
    if workers < 0:
        raise ValueError(f"--decode_workers must be at least 0, got {args.decode_workers!r}")

    def decode():
        if not workers:
            for name in names:
                yield decode_one(name)
            return
        import collections
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:       # in input order, at most 2 * workers files ahead
            ahead, todo = collections.deque(), iter(names)
            for name in todo:
                ahead.append(pool.submit(decode_one, name))
                if len(ahead) >= 2 * workers:
                    yield ahead.popleft().result()
            while ahead:
                yield ahead.popleft().result()

    with FrameStream(model, depth=getattr(args, "depth", 2) or 2, outscale=getattr(args, "outscale", None)) as stream:
        if ext == "jpg":                         # (`same` leaves the stream as it always was)
            stream.jpeg = dict(quality=getattr(args, "jpeg_quality", None) or 95, subsampling=str(getattr(args, "jpeg_subsampling", None) or "420"))
        if ext == "png":
            stream.png = {}
        if niqe_model is not None or references:
            def on_device(frame):
                if niqe_model is not None:
                    scores.append(niqe_model(frame).reshape(()))
                if references:
                    hr = references[next(pending)].to(device=frame.device, non_blocking=True)
                    full_scores.append(torch.stack(score(frame if frame.dim() == 4 else frame[None], hr)).reshape(2))
            stream.on_device = on_device
        # copy=False: the pinned view is encoded before the next result is asked for, i.e. before its slot is submitted to again
        for name, sr_image in zip(names, stream.map(decode(), copy=False)):
            if ext != "same":                    # sr_image is the finished file: written as it came off the device
                name = os.path.splitext(name)[0] + "." + ext
                with open(os.path.join(args.output_dir, name), "wb") as file:
                    file.write(sr_image)
            else:
                Image.fromarray(sr_image).save(os.path.join(args.output_dir, name))
            print(f"SR image save to `{os.path.join(args.output_dir, name)}`")
    if scores:
        values = torch.stack(scores).cpu().tolist()      # the one read-back of the scores
        for name, value in zip(names, values):
            print(f"NIQE {name}: {value:.6f}")
        print(f"NIQE mean: {sum(values) / len(values):.6f}")
    if full_scores:
        values = torch.stack(full_scores).cpu().tolist()      # the one read-back of these scores
        for name, (p, q) in zip(names, values):
            print(f"PSNR/SSIM {name}: {p:.6f} {q:.6f}")
        print(f"PSNR/SSIM mean: {sum(v[0] for v in values) / len(values):.6f} {sum(v[1] for v in values) / len(values):.6f}")


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Using the Real_ESRGAN model generator super-resolution a directory of images.")
    parser.add_argument("--inputs_dir", type=str, required=True, help="Low-resolution image directory.")
    parser.add_argument("--output_dir", type=str, required=True, help="Super-resolution image directory (same file names).")
    parser.add_argument("--weights_path", type=str, required=True, help="Model weights file path.")
    parser.add_argument("--precision", type=str, default=None, choices=["fast", "exact16", "strict"],
                        help="kernel arithmetic; default config.inference_precision = exact16")
    parser.add_argument("--model_type", type=str, default="rrdb", choices=["rrdb", "compact"],
                        help="rrdb: Generator (RRDBNet); compact: upstream's SRVGGNetCompact (realesr-animevideov3 / realesr-general-x4v3)")
    parser.add_argument("--num_conv", type=int, default=16, help="compact: body convs (16 animevideov3, 32 general-x4v3)")
    parser.add_argument("--act_type", type=str, default="prelu", choices=["prelu", "leakyrelu", "relu"], help="compact: activation")
    parser.add_argument("--depth", type=int, default=2, help="frames in flight (FrameStream)")
    parser.add_argument("--outscale", type=float, default=None,
                        help="final upscaling factor (default: the model's own); e.g. 2 writes 2x images from the x4 model")
    parser.add_argument("--keep_mode", action="store_true",
                        help="keep grey (L), RGBA (LA too) and 16-bit grey (I;16) files in their mode instead of converting them to RGB")
    parser.add_argument("--niqe", action="store_true",
                        help="score every RGB frame on the device (native NIQE of the uint8 result) and print the scores and their mean")
    parser.add_argument("--niqe_model_path", type=str, default=None, help="NIQE prior (.mat); default config.niqe_model_path")
    parser.add_argument("--niqe_tail", type=str, default="torch", choices=["torch", "native"],
                        help="--niqe: the features-to-score tail; native = on the device for the frame, no host round trip")
    parser.add_argument("--reference_dir", type=str, default=None,
                        help="ground-truth directory (same file names): PSNR / SSIM of the Y channel of every RGB frame, scored on the device")
    parser.add_argument("--score_channels", type=str, default="y", choices=["y", "rgb"],
                        help="--reference_dir: y = the BT.601 luma level; rgb = PSNR over the three channels, mean of their SSIMs")
    parser.add_argument("--ext", type=str, default="same", choices=["same", "jpg", "png"],
                        help="same: write every file under its own name and format (PIL); jpg / png: frames are encoded on the device, written as <stem>.jpg / <stem>.png")
    parser.add_argument("--jpeg_quality", type=int, default=95, help="--ext jpg: quality 1..100 (the IJG scale)")
    parser.add_argument("--jpeg_subsampling", type=str, default="420", choices=["420", "444"], help="--ext jpg: chroma subsampling")
    parser.add_argument("--decode_workers", type=int, default=0, help="decode the input files on a pool of min(K, 16) threads (0: in line)")
    return parser


if __name__ == "__main__":
    main(get_parser().parse_args())
