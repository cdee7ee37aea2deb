"""Time of one whole RealESRNet step of the trainable compact generator -- forward, fused L1, backward, Adam, EMA
(`train.RealESRNetStep`; synthetic hr / lr, no degradation) -- of the x4 PReLU model with 16 and 32 body convs, `fast`, batch 16, at
HR 256^2 (LR 64^2) and HR 512^2 (LR 128^2).

Three arms in one process, alternated round by round:
  per_tensor   `Adam(model.parameters(), fused=True)`: the only way before `SRVGGNetCompact.flat_parameter()` -- the yardstick;
  flat         `Adam([model.flat_parameter()], fused=True)`: one optimiser tensor, one graph input, one GradScaler check;
  graphed      the flat arm (capturable Adam) under `train.GraphedStep`: the step replayed from one hipGraph.
Each arm owns a model from the same seed.  A round times `steps` steps of each arm with device events after a warm-up of all three;
the figure of an arm is the median over the rounds, the ratios are per_tensor / arm (above 1: the arm is faster than the yardstick).

    python tools/bench_compact_step.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/compact_step.jsonl]

One JSON line per configuration.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import real_esrgan_pytorch_amd as R  # noqa: E402
from real_esrgan_pytorch_amd.train import GraphedStep, RealESRNetStep  # noqa: E402

BATCH, S = 16, 4
ARMS = ("per_tensor", "flat", "graphed")


def make_arm(arm, num_conv, precision):
    torch.manual_seed(0)
    m = R.SRVGGNetCompact(num_conv=num_conv, upscale=S, act_type="prelu", precision=precision, trainable=True).cuda().train()
    ema = R.EMA(m, 0.999)
    ema.register()
    params = m.parameters() if arm == "per_tensor" else [m.flat_parameter()]
    opt = torch.optim.Adam(params, 2e-4, (0.9, 0.99), fused=True, capturable=arm == "graphed")
    scaler = torch.amp.GradScaler("cuda") if precision != "strict" else None
    step = RealESRNetStep(m, ema, opt, scaler, None)
    return GraphedStep(step, warmup=2) if arm == "graphed" else step


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--num-conv", type=int, nargs="*", default=[16, 32])
    ap.add_argument("--size", type=int, nargs="*", default=[64, 128], help="LR edge; HR is 4 x")
    ap.add_argument("--precision", default="fast")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_compact_step: needs the MI355X")
    torch.cuda.set_device(0)
    box = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]}
    for size in args.size:
        gen = torch.Generator(device="cuda").manual_seed(size)
        hr = torch.rand(BATCH, 3, size * S, size * S, device="cuda", generator=gen)
        lr = torch.nn.functional.interpolate(hr, scale_factor=1.0 / S, mode="area")
        for num_conv in args.num_conv:
            steps = {arm: make_arm(arm, num_conv, args.precision) for arm in ARMS}
            for _ in range(max(args.warmup, 3)):         # (GraphedStep: two eager calls, then the capture)
                for arm in ARMS:
                    steps[arm](hr, lr)
            torch.cuda.synchronize()
            assert steps["graphed"]._graph is not None
            times = {arm: [] for arm in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    times[arm].append(time_ms(lambda: steps[arm](hr, lr), args.steps))
            med = {arm: statistics.median(times[arm]) for arm in ARMS}
            line = dict(tool="bench_compact_step", num_conv=num_conv, precision=args.precision, batch=BATCH, lr_size=size, hr_size=size * S,
                        upscale=S, steps=args.steps, warmup=max(args.warmup, 3), rounds=args.rounds, yardstick="per_tensor", **box)
            for arm in ARMS:
                line[f"{arm}_ms"] = round(med[arm], 3)
                line[f"{arm}_ms_min"] = round(min(times[arm]), 3)
                line[f"{arm}_ms_max"] = round(max(times[arm]), 3)
                line[f"{arm}_images_per_s"] = round(BATCH * 1e3 / med[arm], 1)
            line["per_tensor_over_flat"] = round(med["per_tensor"] / med["flat"], 3)
            line["per_tensor_over_graphed"] = round(med["per_tensor"] / med["graphed"], 3)
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            del steps
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
