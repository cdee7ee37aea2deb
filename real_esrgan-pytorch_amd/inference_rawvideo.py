"""Raw YUV 4:2:0 video through the frame path (frames.py, YUV 4:2:0): the shape that sits between the rawvideo pipes of a decoder
and an encoder, with no colour conversion on the host and no dependency beyond this package.

    python -m real_esrgan_pytorch_amd.inference_rawvideo --input in.yuv --output out.yuv --size 1920x1080 --weights_path g.pth \\
        [--pix_fmt yuv420p|nv12|yuv420p10le|p010le --matrix bt601|bt709 --out_pix_fmt ... --out_matrix ... --model_type rrdb|compact
         --num_conv 16 --act_type prelu --precision fast|exact16|strict --depth 2 --outscale 2
         --reference ref.yuv --reference_pix_fmt ... --reference_size WxH]

    ffmpeg -i in.mp4 -f rawvideo -pix_fmt yuv420p - | \\
        python -m real_esrgan_pytorch_amd.inference_rawvideo --input - --output - --size 1920x1080 --model_type compact \\
            --weights_path realesr-animevideov3.pth | \\
        ffmpeg -f rawvideo -pix_fmt yuv420p -s 7680x4320 -r 24 -i - out.mp4

`--input` / `--output`: a file, or `-` for stdin / stdout (every message then goes to stderr).  Frames of W * H * 3 / 2 bytes (8-bit
formats) or W * H * 3 bytes (`yuv420p10le` / `p010le`: a little-endian 16-bit word per sample; use the same `-pix_fmt` on both ffmpeg
pipes) are read one after the other and streamed through `FrameStream(pix_fmt=...)` with `copy=False`; each written frame is
`frames.upscale_yuv420` (`frames.upscale_yuv420p10`) of the frame read, in the same pixel format.  The output size is printed (the encoder has to be told it).
`--out_pix_fmt` / `--out_matrix` (default: the input's) write another format than the one read -- an 8-bit source as 10-bit frames,
BT.601 in and BT.709 out, NV12 surfaces in and planar frames out: each written frame is `frames.upscale_frames` of the frame read
(frames.py, MIXED FRAME FORMATS); the second ffmpeg pipe takes the output's `-pix_fmt`.
A trailing partial frame is an error that names its byte count.  The model is built and the checkpoint loaded as `inference.py`
does (inference_frames.build_model).

`--reference ref.yuv`: raw video of the OUTPUT's size and bit depth, in `--reference_pix_fmt` (default: the output's format).  It is
read frame by frame next to the input and uploaded without blocking; every written frame is scored against its reference frame where
the last kernel left it (`FrameStream.on_device`, `image_quality_assessment.full_ref_yuv_native`: the stored Y, Cb and Cr planes, no
conversion to RGB, no crop), and the scores are read back once, at the end.  One line per frame goes to stderr (stdout may be the
video), `PSNR y/u/v/avg SSIM y/u/v <index>: <dB> <dB> <dB> <dB> <ssim> <ssim> <ssim>`, then the same with `mean` for the index; `avg` is
the PSNR over all 1.5 W H samples (ffmpeg's "average").  Raised before any frame is computed, each naming its cause: a reference with
fewer frames than the input (both regular files; with a pipe on either side, when the reference runs out), a reference that is not
whole frames of the output's size, a `--reference_size` that is not the output's, a reference of another bit depth, and `--reference`
with an rgb24 output.
"""
import argparse
import collections
import contextlib
import os
import re
import sys

import numpy as np
import torch

from . import config
from .frames import FrameStream, yuv420_output_size
from .inference_frames import build_model

PIX_FMTS = {"yuv420p": "i420", "nv12": "nv12", "yuv420p10le": "i420p10", "p010le": "p010"}      # the rawvideo names -> frames.py's layouts
WORD = {"i420": np.dtype(np.uint8), "nv12": np.dtype(np.uint8), "i420p10": np.dtype("<u2"), "p010": np.dtype("<u2")}   # a sample's word


def parse_size(text: str):
    """'WxH' -> (W, H), both even and positive."""
    m = re.fullmatch(r"(\d+)[xX](\d+)", text or "")
    if not m:
        raise ValueError(f"--size must be WxH, got {text!r}")
    w, h = int(m.group(1)), int(m.group(2))
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError(f"--size: a 4:2:0 frame has an even, positive width and height, got {w}x{h}")
    return w, h


def frame_bytes(w: int, h: int, word=np.uint8) -> int:
    """Bytes of one W x H 4:2:0 frame of `word` samples: W * H * 3 / 2 for bytes, W * H * 3 for 16-bit words."""
    return w * h * 3 // 2 * np.dtype(word).itemsize


def read_frames(stream, w: int, h: int, word=np.uint8):
    """The [3H/2, W] frames (uint8, or little-endian uint16 for `word=WORD["i420p10"]`) of a byte stream; ValueError for a
    trailing partial frame."""
    nbytes = frame_bytes(w, h, word)
    index = 0
    while True:
        buf = bytearray()
        while len(buf) < nbytes:                       # a pipe hands out what it has: read until the frame is whole
            chunk = stream.read(nbytes - len(buf))
            if not chunk:
                break
            buf += chunk
        if not buf:
            return
        if len(buf) != nbytes:
            raise ValueError(f"frame {index}: {len(buf)} trailing bytes, a {w}x{h} 4:2:0 frame has {nbytes}")
        yield np.frombuffer(buf, dtype=word).astype(np.dtype(word).newbyteorder("="), copy=False).reshape(h * 3 // 2, w)
        index += 1


def formats(args):
    """(pix_fmt, matrix, out_pix_fmt, out_matrix) of the arguments, rawvideo names: the output's default to the input's."""
    pix_fmt = getattr(args, "pix_fmt", "yuv420p") or "yuv420p"
    matrix = getattr(args, "matrix", "bt601") or "bt601"
    out_pix_fmt = getattr(args, "out_pix_fmt", None) or pix_fmt
    for flag, name in (("--pix_fmt", pix_fmt), ("--out_pix_fmt", out_pix_fmt)):
        if name not in PIX_FMTS:
            raise ValueError(f"{flag} must be one of {sorted(PIX_FMTS)}, got {name!r}")
    return pix_fmt, matrix, out_pix_fmt, getattr(args, "out_matrix", None) or matrix


SCORE_LINE = "PSNR y/u/v/avg SSIM y/u/v"


def reference_plan(args, out_pix_fmt: str, out_w: int, out_h: int, in_frame_bytes: int):
    """What `--reference` asks for, checked before any frame is computed -> (path, layout, word) or None without the flag."""
    path = getattr(args, "reference", None)
    if not path:
        return None
    name = getattr(args, "reference_pix_fmt", None) or out_pix_fmt
    if name not in PIX_FMTS:
        raise ValueError(f"--reference_pix_fmt must be one of {sorted(PIX_FMTS)}, got {name!r}")
    layout, word = PIX_FMTS[name], WORD[PIX_FMTS[name]]
    if word != WORD[PIX_FMTS[out_pix_fmt]]:
        raise ValueError(f"--reference: the reference is {name} ({8 if word.itemsize == 1 else 10} bits), the output {out_pix_fmt}: both must have one bit depth")
    size = getattr(args, "reference_size", None)
    if size and parse_size(size) != (out_w, out_h):
        raise ValueError(f"--reference: the reference is {size}, the output {out_w}x{out_h}: the reference must have the output's size")
    if path != "-" and os.path.isfile(path):
        nbytes, have = frame_bytes(out_w, out_h, word), os.path.getsize(path)
        if have % nbytes:
            raise ValueError(f"--reference: `{path}` has {have} bytes, not whole {out_w}x{out_h} {name} frames of {nbytes}: the reference must have the output's size")
        if args.input != "-" and os.path.isfile(args.input) and have // nbytes < os.path.getsize(args.input) // in_frame_bytes:
            raise ValueError(f"--reference: `{path}` has {have // nbytes} frames, the input {os.path.getsize(args.input) // in_frame_bytes}: the reference is shorter than the input")
    return path, layout, word


def main(args) -> int:
    w, h = parse_size(args.size)
    if getattr(args, "reference", None) and (getattr(args, "out_pix_fmt", None) or getattr(args, "pix_fmt", None)) == "rgb24":
        raise ValueError("--reference scores YUV planes: it cannot be used with an rgb24 output")
    pix_fmt, matrix, out_pix_fmt, out_matrix = formats(args)
    layout, out_layout = PIX_FMTS[pix_fmt], PIX_FMTS[out_pix_fmt]
    word, out_word = WORD[layout], WORD[out_layout]
    log = sys.stderr if args.output == "-" else sys.stdout
    torch.cuda.set_device(config.device)
    with contextlib.redirect_stdout(log):
        model = build_model(args)
    outscale = getattr(args, "outscale", None)
    out_h, out_w = yuv420_output_size(h, w, model.upscale_factor, outscale, "inference_rawvideo")
    print(f"Output size {out_w}x{out_h} ({out_pix_fmt}, {frame_bytes(out_w, out_h, out_word)} bytes per frame).", file=log)
    reference = reference_plan(args, out_pix_fmt, out_w, out_h, frame_bytes(w, h, word))
    count = 0
    scores = []                                 # --reference: one [7] device tensor per frame, read once at the end
    with contextlib.ExitStack() as stack:
        src = sys.stdin.buffer if args.input == "-" else stack.enter_context(open(args.input, "rb"))
        dst = sys.stdout.buffer if args.output == "-" else stack.enter_context(open(args.output, "wb"))
        stream = stack.enter_context(FrameStream(model, depth=getattr(args, "depth", 2) or 2, outscale=outscale, pix_fmt=layout,
                                                 matrix=matrix, out_pix_fmt=out_layout, out_matrix=out_matrix))
        # copy=False: the pinned view is written out before the next result is asked for, i.e. before its slot is submitted to again
        frames = read_frames(src, w, h, word)
        if reference:
            from .image_quality_assessment import full_ref_yuv_native
            ref_src = sys.stdin.buffer if reference[0] == "-" else stack.enter_context(open(reference[0], "rb"))
            ref_frames = read_frames(ref_src, out_w, out_h, reference[2])
            waiting = collections.deque()       # pinned reference frames, in input order: on_device sees the results in that order

            def paired(frames=frames):
                for index, frame in enumerate(frames):
                    ref = next(ref_frames, None)
                    if ref is None:
                        raise ValueError(f"--reference: `{reference[0]}` ends before frame {index} of the input: the reference is shorter than the input")
                    waiting.append(torch.from_numpy(np.ascontiguousarray(ref)).pin_memory())
                    yield frame

            def on_device(frame):
                hr = waiting.popleft().to(device=frame.device, non_blocking=True)[None]
                scores.append(torch.stack(full_ref_yuv_native(frame if frame.dim() == 3 else frame[None], hr, out_layout, reference[1])).reshape(7))
            stream.on_device = on_device
            frames = paired()
        for sr in stream.map(frames, copy=False):
            dst.write(sr.astype(out_word, copy=False).data)     # (little-endian words: a view on every host this runs on)
            count += 1
        dst.flush()
    print(f"{count} frames written to `{args.output}`.", file=log)
    if scores:
        values = torch.stack(scores).cpu().tolist()         # the one read-back of the scores
        for index, row in enumerate(values):
            print(f"{SCORE_LINE} {index}: " + " ".join(f"{v:.6f}" for v in row), file=sys.stderr)
        print(f"{SCORE_LINE} mean: " + " ".join(f"{sum(r[i] for r in values) / len(values):.6f}" for i in range(7)), file=sys.stderr)
    return count


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Using the Real_ESRGAN model generator super-resolution raw YUV 4:2:0 video.")
    parser.add_argument("--input", type=str, required=True, help="Raw video file, or - for stdin.")
    parser.add_argument("--output", type=str, required=True, help="Raw video file, or - for stdout.")
    parser.add_argument("--size", type=str, required=True, help="Input frame size WxH (both even), e.g. 1920x1080.")
    parser.add_argument("--pix_fmt", type=str, default="yuv420p", choices=sorted(PIX_FMTS), help="pixel format of the input (and of the output, unless --out_pix_fmt)")
    parser.add_argument("--matrix", type=str, default="bt601", choices=["bt601", "bt709"], help="colour matrix (studio range)")
    parser.add_argument("--out_pix_fmt", type=str, default=None, choices=sorted(PIX_FMTS), help="pixel format of the output (default: --pix_fmt)")
    parser.add_argument("--out_matrix", type=str, default=None, choices=["bt601", "bt709"], help="colour matrix of the output (default: --matrix)")
    parser.add_argument("--weights_path", type=str, required=True, help="Model weights file path.")
    parser.add_argument("--precision", type=str, default=None, choices=["fast", "exact16", "strict"],
                        help="kernel arithmetic; default config.inference_precision = exact16")
    parser.add_argument("--model_type", type=str, default="rrdb", choices=["rrdb", "compact"],
                        help="rrdb: Generator (RRDBNet); compact: upstream's SRVGGNetCompact (realesr-animevideov3 / realesr-general-x4v3)")
    parser.add_argument("--num_conv", type=int, default=16, help="compact: body convs (16 animevideov3, 32 general-x4v3)")
    parser.add_argument("--act_type", type=str, default="prelu", choices=["prelu", "leakyrelu", "relu"], help="compact: activation")
    parser.add_argument("--depth", type=int, default=2, help="frames in flight (FrameStream)")
    parser.add_argument("--outscale", type=float, default=None,
                        help="final upscaling factor (default: the model's own); the output width and height must come out even")
    parser.add_argument("--reference", type=str, default=None,
                        help="raw video of the output's size and depth: PSNR / SSIM of the Y, U and V planes of every frame, scored on the device, printed to stderr")
    parser.add_argument("--reference_pix_fmt", type=str, default=None, choices=sorted(PIX_FMTS), help="pixel format of --reference (default: the output's)")
    parser.add_argument("--reference_size", type=str, default=None, help="WxH of --reference, if you want it checked against the output size")
    return parser


if __name__ == "__main__":
    main(get_parser().parse_args())
