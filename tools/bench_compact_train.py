"""Time of one training step's generator part -- forward + backward -- of the trainable compact generator
(SRVGGNetCompact(num_conv 16 / 32, upscale 4, "prelu", trainable=True)) at 16 x 3 x 64^2 and 16 x 3 x 128^2, `fast` and `strict`.

The yardstick is not this code: it is upstream's module (tests.compact_oracle.UpstreamCompact) on the same GPU through PyTorch-ROCm's
own kernels and autograd -- torch.autocast(float16) on channels_last tensors for `fast`, plain fp32 for `strict`.  Both run in one
process, alternating: a round times `steps` forward + backward passes of the one, then of the other, with device events, after a warm-up
of both; the figure reported for each is the median over the rounds, and their ratio (PyTorch / native: above 1 = the native pass is
faster).  The loss is a sum with a fixed random cotangent; parameter gradients and the input's gradient are all computed on both sides.

    python tools/bench_compact_train.py [--steps 10] [--warmup 5] [--rounds 7] [--out profiles/compact_train.jsonl]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_compact_train.py --native-only --num-conv 16 --size 128 --precision fast

--native-only runs the native pass of the chosen cases alone (warm-up + one round): the per-kernel split of a profiler run is then the
native pass's.  One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from tests.compact_oracle import UpstreamCompact  # noqa: E402

BATCH, S = 16, 4


def flop_per_step(num_conv, size):
    """Forward + backward-data + weight gradient: 3 x the forward's multiply-adds x 2 (conv 0 has no backward-data worth counting)."""
    return 3 * 2.0 * 9 * BATCH * size * size * (3 * 64 + num_conv * 64 * 64 + 64 * 3 * S * S)


def native_step(num_conv, precision, x, gy):
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, act_type="prelu", precision=precision, trainable=True).cuda().train()
    xi = x.clone().requires_grad_()

    def step():
        m.zero_grad(set_to_none=True)
        xi.grad = None
        m(xi).backward(gy)
    return step


def torch_step(num_conv, precision, x, gy):
    torch.manual_seed(0)
    m = UpstreamCompact(num_conv, S, "prelu").cuda().train()

    def forward(xi):
        h = xi
        for layer in m.body:
            h = layer(h)
        return m.upsampler(h) + torch.nn.functional.interpolate(xi, scale_factor=S, mode="nearest")
    if precision == "fast":
        m = m.to(memory_format=torch.channels_last)
        xi = x.clone().to(memory_format=torch.channels_last).requires_grad_()
        gyc = gy.to(memory_format=torch.channels_last)

        def step():
            m.zero_grad(set_to_none=True)
            xi.grad = None
            with torch.autocast("cuda", dtype=torch.float16):
                y = forward(xi)
            y.backward(gyc.to(y.dtype))
    else:
        xi = x.clone().requires_grad_()

        def step():
            m.zero_grad(set_to_none=True)
            xi.grad = None
            forward(xi).backward(gy)
    return step


def time_ms(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--num-conv", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--size", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--precision", nargs="*", default=["fast", "strict"])
    ap.add_argument("--native-only", action="store_true", help="the native pass alone, one round (for a profiler run)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_compact_train: needs the MI355X")
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    for size in args.size:
        gen = torch.Generator(device="cuda").manual_seed(size)
        x = torch.rand(BATCH, 3, size, size, device="cuda", generator=gen)
        gy = torch.randn(BATCH, 3, size * S, size * S, device="cuda", generator=gen) * 1e-3
        for num_conv in args.num_conv:
            for precision in args.precision:
                native = native_step(num_conv, precision, x, gy)
                other = None if args.native_only else torch_step(num_conv, precision, x, gy)
                for _ in range(args.warmup):
                    native()
                    if other:
                        other()
                torch.cuda.synchronize()
                t_native, t_other = [], []
                for _ in range(1 if args.native_only else args.rounds):
                    t_native.append(time_ms(native, args.steps))
                    if other:
                        t_other.append(time_ms(other, args.steps))
                ms = statistics.median(t_native)
                line = dict(tool="bench_compact_train", num_conv=num_conv, precision=precision, batch=BATCH, lr_size=size, upscale=S,
                            native_ms=round(ms, 3), native_ms_min=round(min(t_native), 3), native_ms_max=round(max(t_native), 3),
                            native_tflops=round(flop_per_step(num_conv, size) / (ms * 1e-3) / 1e12, 1),
                            native_images_per_s=round(BATCH * 1e3 / ms, 1), steps=args.steps, warmup=args.warmup, rounds=len(t_native), **box)
                if other:
                    oms = statistics.median(t_other)
                    line.update(pytorch_ms=round(oms, 3), pytorch_ms_min=round(min(t_other), 3), pytorch_ms_max=round(max(t_other), 3),
                                pytorch_over_native=round(oms / ms, 3),
                                yardstick="UpstreamCompact, torch autograd, " + ("autocast f16 channels_last" if precision == "fast" else "fp32"))
                print(json.dumps(line), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                del native, other
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
