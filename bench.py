#!/usr/bin/env python3
"""bench.py -- x4 SR train images/sec (256x256 -> 1024x1024) on N MI355X, one process per GPU.

    python bench.py --gpus N --steps K --warmup W        (N > 1 without a launcher: starts its N ranks itself, see self_launch)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --full                               (everything else the line can carry, see below)
    python bench.py --dump-outputs DIR                   (also write what the last timed step computed, DIR/<name>.npy)

A "step" is one RealESRNet optimisation step (reference train_realesrnet.py:258-413 loop body) on a
batch of synthetic HR tiles already resident in HBM: second-order degradation -> RRDBNet forward ->
L1 -> backward (data + weight gradients) -> RCCL all-reduce of the flat gradient arena (N > 1) ->
fused Adam -> EMA.  Rank 0 prints ONE JSON line: `metric`, `value`, `unit`, `ms_per_step` (K timed steps
after W warm-up steps) and the workload.  A plain run does only that.  With --full the line also carries
`roofline` (dominant MFMA kernel, timed live with events on the launch stream, one extra step), `parity_mode`
(exact16 sub-runs and probes), `other_configs`, `box_reference`, `power`, `host` and `cpu_baseline`
(the CPU oracle timed on the host cores, N = 1 only).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as CHILDREN through torch.distributed.run (one rank per GPU,
    rendezvous on 127.0.0.1 at a free port), relay their output -- rank 0's single JSON line included -- and return the launcher's exit
    code.  Runs before this process has made any HIP call, and starts children rather than replacing itself (a process that has
    initialised the GPU must never exec, and this one stays clean anyway)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write(f"bench.py: no launcher in the environment -- starting {n} ranks: {' '.join(cmd)}\n")
    sys.stderr.flush()
    return subprocess.call(cmd, env=env)



def _gpus_from_argv(argv):
    """--gpus N / --gpus=N without argparse (and without torch): 1 when absent or malformed (argparse reports that later)."""
    for i, a in enumerate(argv):
        try:
            if a == "--gpus" and i + 1 < len(argv):
                return int(argv[i + 1])
            if a.startswith("--gpus="):
                return int(a.split("=", 1)[1])
        except ValueError:
            return 1
    return 1


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and _gpus_from_argv(sys.argv[1:]) > 1:
    # plain `python bench.py --gpus N`: hand over to N ranks BEFORE torch is even imported -- this process never loads HIP, and the launch
    # costs one interpreter start-up with torch less
    raise SystemExit(self_launch(_gpus_from_argv(sys.argv[1:])))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MAC_PER_LR_PX = 17_926_848          # generator x4 forward MACs per LR pixel
PEAK_F16_TFLOPS = 2500.0            # dense f16/bf16 MFMA peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0              # HBM3E peak (spec; ~6300 achievable), MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
DUMP_SAMPLE = 1 << 21               # --dump-outputs: elements kept of a larger array (8 MB each; the six arrays of a step stay under 64 MB)


def parse():
    ap = _parser()
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.lr_size is None:
        args.lr_size = 64 if args.gan else 256
    if not args.full:
        # a plain run does what its headline needs: set-up, warm-up, the timed steps, the outputs, the line
        args.no_cpu_baseline = args.no_parity_mode = args.no_other_configs = args.no_probe = args.no_sustained = True
    return args


def _parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU per step: 16 = BASELINE config 4's 128 images over 8 GPUs (the reference's own batch_size is 48 per process, "
                         "config.py:90 -- reported under other_configs.reference_batch48; 8..48 measured within 8 %% of each other)")
    ap.add_argument("--lr-size", type=int, default=None, help="LR tile edge; HR = 4x (default: 256 -> 1024, the headline; 64 -> 256 with --gan)")
    ap.add_argument("--precision", default="fast", choices=["fast", "exact16", "strict"])
    ap.add_argument("--no-degradation", action="store_true", help="debug only: feed pre-degraded LR tiles")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity-mode", action="store_true", help="skip the exact16 sub-run (parity_mode record)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short runs of the other BASELINE.json configurations (2, 3, 4, 5) reported under other_configs")
    ap.add_argument("--gan", action="store_true",
                    help="BASELINE config 4 instead of the headline: the RealESRGAN step (generator update with the discriminator "
                         "frozen, USM on sr, VGG19 term, then two discriminator backwards; train_realesrgan.py:459-521), "
                         "16 images per GPU, HR 400^2 tiles cropped to 256^2 (LR 64^2) unless --lr-size says otherwise")
    ap.add_argument("--noise-data", action="store_true",
                    help="uniform-noise HR tiles (SURVEY 8d's literal torch.rand tiles) instead of the image-like default: on those the "
                         "first Adam step saturates the output clamp, the backward pass carries zero gradients and the matrix kernels "
                         "run 10-20 %% faster than on real gradients (DESIGN.md section 5)")
    ap.add_argument("--per-tensor-adam", action="store_true", help="optimizer over the 702 per-tensor Parameters instead of the flat arena")
    ap.add_argument("--no-probe", action="store_true", help="skip the in-situ roofline step")
    ap.add_argument("--no-sustained", action="store_true", help="skip the 3 s measurement of this box's power-cap frontier (kernel traces: it is ~13 K launches)")
    ap.add_argument("--centre-output", action="store_true",
                    help="conv4.bias + 0.5 before the run (what the config-3 probe does): at LR 64^2 a random init whose first Adam step overshoots the "
                         "training-time clamp leaves a step with zero gradients, which draws less power and times ~8 %% faster than a real one")
    ap.add_argument("--isolated-probe", action="store_true", help="also time every conv shape back-to-back in isolation")
    ap.add_argument("--single-policy", action="store_true",
                    help="N > 1: time only the exchange policy the environment selects (default: BOTH -- sequential, then RESR_DP_OVERLAP=1 + "
                         "RESR_CHAIN_CUS_PER_XCD=31 -- K timed steps each, the better one is `value`, both under dist.policies)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: parity_mode (exact16 sub-runs, probes), other_configs, cpu_baseline, the in-situ "
                         "roofline step and the degradation record, box_reference (~3 s frontier measurement), power, host and "
                         "unclamped_output_fraction; the --no-* options above switch parts of it off.  Without it: set-up, warm-up, the timed "
                         "steps and the result line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32; arrays above "
                         f"{DUMP_SAMPLE} elements as a fixed seeded sample of that many; rank 0)")
    return ap


def ensure_built():
    lib = os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "libresr_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__
        __graft_entry__.build()


def conv_launch_table(batch, lr, n_blocks=23):
    """(cin, cout, cout_pad, res_mult, flags) -> launches per train step, by kernel instance.
    Mirrors generator.hip: forward convs + mirrored backward-data passes (weight-gradient kernels are
    a different instance and are listed in DESIGN.md)."""
    nrdb = 3 * n_blocks
    t = {}

    def add(cin, cout, cout_pad, mult, count):
        t[(cin, cout, cout_pad, mult)] = t.get((cin, cout, cout_pad, mult), 0) + count

    for cin in (64, 96, 128, 160):
        add(cin, 32, 32, 1, 2 * nrdb)       # conv1..4 forward + backward passes g_o4..g_o1
    add(192, 64, 64, 1, 2 * nrdb)           # conv5 forward + backward pass g_x
    add(32, 64, 64, 1, 1)                   # conv1 forward (3 real input channels, padded to 32)
    add(64, 64, 64, 1, 2)                   # conv2 fwd + bwd
    add(64, 64, 64, 2, 2)                   # upsampling1 fwd + bwd
    add(64, 64, 64, 4, 4)                   # upsampling2 + conv3, fwd + bwd
    add(64, 3, 32, 4, 1)                    # conv4 forward
    add(32, 64, 64, 4, 1)                   # conv4 backward-data
    return t


def probe_conv_kernels(batch, lr, dtype_name, reps=8):
    """Time every conv3x3 launch shape of the step on the launch stream with events; returns rows."""
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    dtype = L.RESR_F16 if dtype_name == "fast" else L.RESR_F32
    tdt = torch.float16 if dtype == L.RESR_F16 else torch.float32
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for (cin, cout, cout_pad, mult), count in conv_launch_table(batch, lr).items():
        h = w = lr * mult
        x = (torch.rand(batch, h, w, cin, device="cuda", generator=gen) - 0.5).to(tdt)
        y = torch.empty(batch, h, w, cout_pad, device="cuda", dtype=tdt)
        yn = torch.empty(batch, max(cout, 1), h, w, device="cuda", dtype=torch.float32) if cout < 4 else None
        mt = cout_pad // 32
        # timing only: any finite weights in packed order will do (+ one tap of prefetch slack)
        packed = ((torch.rand(((cin // 32) * 9 * mt * 1024 + 8192,), device="cuda", generator=gen) - 0.5) * 0.1).to(tdt)
        flags = L.CONV_LRELU | (L.CONV_OUT_NCHW_F32 | L.CONV_CLAMP01 if yn is not None else 0)
        d = L.ConvDesc(batch, h, w, cin, cin, cin, 0, cout, cout_pad, cout_pad, 0, 0, 0, dtype, flags,
                       1.0, 1.0, 1.0, 1.0, 0.2)
        out = yn if yn is not None else y
        st = L.stream_ptr()

        def launch():
            L.check(lib.resr_conv3x3(C.byref(d), L.ptr(x), None, L.ptr(packed), None, None, None, None, L.ptr(out),
                                     None, st), "resr_conv3x3")
        for _ in range(2):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        flop = 2.0 * 9 * cin * cout * batch * h * w
        # label only (the library picks the instantiation): fast mode = producer/consumer kernel, strict = one-role kernel
        inst = f"conv3x3_ws_kernel<f16,mt={mt}>" if dtype == L.RESR_F16 else f"conv3x3_kernel<f32,{mt},2,4>"
        rows.append({"kernel": inst, "cin": cin, "cout": cout, "res": h, "launches_per_step": count,
                     "ms": ms, "tflops": flop / ms / 1e9, "flop": flop})
        del x, y, yn, packed
    return rows


def kernel_sources_sha16():
    """sha256 over the sources that decide the hot kernels' traffic (the conv / weight-gradient kernels and the generator's
    launch plan): a PMC measurement is only quoted for the build it was taken on."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for path in sorted(glob.glob(os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "conv3x3*.h*")) +
                       glob.glob(os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "wgrad.h*")) +
                       [os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "generator.hip")]):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def degrade_sources_sha16():
    """sha256 over the sources that decide the degradation stage's traffic (its kernels and its launch plan)."""
    import hashlib
    h = hashlib.sha256()
    for path in (os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc", "degrade.hip"), os.path.join(ROOT, "real_esrgan-pytorch_amd", "degrade.py"),
                 os.path.join(ROOT, "real_esrgan-pytorch_amd", "imgproc.py")):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def degradation_roofline(degrade, hr, batch, step_ms, step_ms_no_degradation):
    """The degradation stage against the HBM roofline: its kernels alone on their side stream, `ms` per batch by HIP
    events on THAT stream over five batches (plans differ from batch to batch: random resize factors and noise kinds), HBM bytes
    per batch from the committed PMC passes of this command (profiles/r*_pmc_traffic_b<batch>.json `degradation_stage`, quoted
    only while the hash of the degradation sources matches), and what the stage costs the step on this box: the timed step against
    the same step fed pre-degraded tiles."""
    import glob
    st = degrade.stream
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    keep = []
    reps = 5
    with torch.cuda.stream(st):
        e0.record(st)
    for _ in range(reps):
        keep.append(degrade._enqueue(hr))
    with torch.cuda.stream(st):
        e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del keep
    rec = {"bound": "hbm", "peak": PEAK_HBM_GBS, "unit": "GB/s", "ms_per_batch_alone": round(ms, 3),
           "how": f"{reps} batches back to back on the side stream, nothing else running; HIP events on that stream",
           "step_ms_with": round(step_ms, 2), "step_ms_without": round(step_ms_no_degradation, 2) if step_ms_no_degradation else None,
           "step_delta_ms": round(step_ms - step_ms_no_degradation, 2) if step_ms_no_degradation else None}
    sha, stale = degrade_sources_sha16(), None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic_b{batch}.json")), reverse=True):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        if "degradation_stage" not in d:
            continue
        if d.get("degrade_sha16") != sha:
            stale = stale or f"{os.path.basename(path)} was measured on another build of the degradation stage: not quoted"
            continue
        b = d["degradation_stage"]["hbm_bytes_per_batch"]
        rec.update(traffic=b, traffic_source=os.path.basename(path), achieved=round(b / ms / 1e6, 1), frac=round(b / ms / 1e6 / PEAK_HBM_GBS, 4))
        break
    else:
        rec.update(traffic=None, traffic_note=stale or "no PMC file with a degradation_stage record for this batch size", achieved=None, frac=None)
    return rec


def pmc_traffic(kernel, batch):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes of this same command
    (profiles/r*_pmc_traffic_b<batch>.json, made by tools/pmc_traffic.py through tools/profile_round.sh: FETCH_SIZE and
    WRITE_SIZE in separate runs, FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md).  PMC counters cannot be read
    from inside the process, so this is the last measured value for this batch size -- and only if the file was made on THIS
    build of the kernels (its "csrc_sha16" equals the hash of the current sources); otherwise None and the reason."""
    import glob
    sha = kernel_sources_sha16()
    stale = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic_b{batch}.json")), reverse=True):
        try:
            d = json.load(open(path))
            if kernel in d:
                if d.get("csrc_sha16") == sha:
                    return d[kernel]["hbm_bytes_per_launch"], os.path.basename(path)
                stale = stale or f"{os.path.basename(path)} was measured on another build of the kernels (csrc_sha16 {d.get('csrc_sha16')} != {sha}): not quoted"
        except Exception:
            pass
    return None, stale


_LIVE_FRONTIER = None


def measure_sustained_frontier(seconds=1.5):
    """The power-cap frontier of THIS board, measured in this process before the timed steps (resr_debug_sustained: 256 workgroups
    back to back for `seconds` per arm, last third timed): the matrix waves alone, and the matrix waves next to an LDS-DMA stream.
    The box-to-box spread of one build is +-5 %: a frontier from another box (the committed profiles/ file) cannot price this
    run's kernels.  ~3 s; stored for sustained_frontier()."""
    global _LIVE_FRONTIER
    import real_esrgan_pytorch_amd as R
    L = R._lib
    try:
        src = torch.ones(1 << 29, dtype=torch.uint8, device="cuda")       # 512 MB: beyond the Infinity Cache
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        tb, pf = C.c_double(0), C.c_double(0)
        L.check(L.lib().resr_debug_sustained(2, seconds, L.ptr(src), src.numel(), L.ptr(cnt), C.byref(tb), C.byref(pf), L.stream_ptr()), "sustained")
        alone = pf.value
        L.check(L.lib().resr_debug_sustained(3, seconds, L.ptr(src), src.numel(), L.ptr(cnt), C.byref(tb), C.byref(pf), L.stream_ptr()), "sustained")
        _LIVE_FRONTIER = (alone, tb.value, pf.value, f"this box, this process (resr_debug_sustained, each arm held {seconds} s)")
        del src, cnt
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        _LIVE_FRONTIER = None
        sys.stderr.write(f"sustained frontier not measured: {e!r}\n")
    return _LIVE_FRONTIER


def sustained_frontier():
    """(matrix PFLOP/s alone, stream TB/s, matrix PFLOP/s next to that stream, source): the live measurement of this box
    (measure_sustained_frontier) when there is one, else the committed run of tools/micro/sustained.hip
    (profiles/r*_micro_sustained.txt, another box), or None."""
    import glob
    import re
    if _LIVE_FRONTIER:
        return _LIVE_FRONTIER
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_micro_sustained.txt")), reverse=True):
        try:
            alone = both_s = both_m = None
            for line in open(path):
                if "sustained" not in line:
                    continue
                m = re.search(r"stream\s+([0-9.]+) TB/s\s+matrix\s+([0-9.]+) PFLOP/s", line)
                if not m:
                    continue
                st, mx = float(m.group(1)), float(m.group(2))
                if st == 0.0:
                    alone = mx
                elif mx > 0.0:
                    both_s, both_m = st, mx
            if alone and both_s:
                return alone, both_s, both_m, "profiles/" + os.path.basename(path) + " (tools/micro/sustained.hip, each arm held 1.5 s; an EARLIER box)"
        except Exception:
            pass
    return None


def kernel_name(kid):
    if kid >= 50000:
        k = kid - 50000
        if k == 200:
            return "wgrad_quad_kernel<f16>"
        if k == 500:
            return "wgrad_quad_kernel<f16x2>"
        if k >= 300:
            return f"wgrad_kernel<f16x2,{k % 100}>"
        return f"wgrad_kernel<{'f32' if k >= 100 else 'f16'},{k % 100}>"
    if kid >= 26000:  # exact16, the cout-32 passes of a dense block as one chained launch
        k = kid - 26000
        return f"conv3x3_ws_kernel<f16x2,{k // 100},{(k // 10) % 10},{k % 10},chain>"
    if kid >= 25000:  # exact16: the same kernel on hi/lo f16 pairs, three stages per chunk
        k = kid - 25000
        return f"conv3x3_ws_kernel<f16x2,{k // 100},{(k // 10) % 10},{k % 10}>"
    if kid >= 24000:  # the same kernel running the four cout-32 passes of a dense block as one chained launch
        k = kid - 24000
        return f"conv3x3_ws_kernel<f16,{k // 100},{(k // 10) % 10},{k % 10},chain>"
    if kid >= 20000:  # fast-mode producer/consumer kernel: <f16, MT, NT, consumer waves>
        k = kid - 20000
        return f"conv3x3_ws_kernel<f16,{k // 100},{(k // 10) % 10},{k % 10}>"
    t = "f32" if kid >= 10000 else "f16"
    k = kid % 10000
    return f"conv3x3_kernel<{t},{k // 100},{(k // 10) % 10},{k % 10}>"


def precision_is_f16(res):
    return res.get("precision") in ("fast", "exact16")


class PowerSampler:
    """Board power and shader clock of the current GPU read from its hwmon files (amdgpu: power1_input in uW, power1_cap,
    freq1_input = sclk in Hz) every 50 ms on a side thread while the timed steps run: the step sits at the board's power
    cap, and this puts the evidence into the driver-run line.  Best effort: None where the files are
    absent or unreadable."""

    def __init__(self):
        import glob
        import threading
        self.dir = None
        try:
            p = torch.cuda.get_device_properties(torch.cuda.current_device())
            bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}."
            for d in glob.glob("/sys/class/drm/card*/device"):
                if os.path.basename(os.path.realpath(d)).startswith(bdf):
                    h = glob.glob(os.path.join(d, "hwmon", "hwmon*"))
                    if h and os.path.exists(os.path.join(h[0], "power1_input")):
                        self.dir = h[0]
        except Exception:
            self.dir = None
        self.samples = []
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True) if self.dir else None

    def _read(self, name):
        with open(os.path.join(self.dir, name)) as f:
            return float(f.read().strip())

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append((self._read("power1_input") / 1e6, self._read("freq1_input") / 1e6))
            except Exception:
                pass
            self._stop.wait(0.05)

    def __enter__(self):
        if self._thread:
            self._thread.start()
        return self

    def __exit__(self, *exc):
        if self._thread:
            self._stop.set()
            self._thread.join()

    def summary(self):
        if not self.samples:
            return None
        w = [s[0] for s in self.samples]
        f = [s[1] for s in self.samples]
        cap = None
        try:
            cap = self._read("power1_cap") / 1e6
        except Exception:
            pass
        return {"avg_w": round(sum(w) / len(w), 1), "max_w": round(max(w), 1), "cap_w": cap, "sclk_mhz_avg": round(sum(f) / len(f)),
                "samples": len(w), "source": "amdgpu hwmon power1_input / freq1_input, 50 ms, over the timed steps"}


def roofline_in_situ(step_fn, precision, batch):
    """One extra (untimed) train step with every conv3x3 / wgrad launch bracketed by HIP events on its launch stream
    (resr_profile_begin/end).  The dominant kernel is the instance with the largest summed duration; achieved =
    sum of its launches' algorithmic FLOP (2*9*cin*cout*pixels each) / sum of their durations."""
    import real_esrgan_pytorch_amd as R
    L = R._lib
    lib = L.lib()
    lib.resr_profile_begin()
    step_fn()
    torch.cuda.synchronize()
    cap = 8192
    buf = (L.ProfEntry * cap)()
    n = int(lib.resr_profile_end(C.cast(buf, C.c_void_p), cap))
    by = {}
    for i in range(min(n, cap)):
        b = by.setdefault(kernel_name(buf[i].kernel_id), {"t": 0.0, "f": 0.0, "n": 0, "b": 0.0})
        b["t"] += buf[i].ms
        b["f"] += buf[i].flop
        b["b"] += buf[i].bytes
        b["n"] += 1
    name, b = max(by.items(), key=lambda kv: kv[1]["t"])
    achieved = b["f"] / b["t"] / 1e9
    peak = PEAK_F32_TFLOPS if precision == "strict" else PEAK_F16_TFLOPS
    traffic, src = pmc_traffic(name, batch)
    r = {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
         "frac": round(achieved / peak, 4), "traffic": traffic,
         "avg_launch_ms": round(b["t"] / b["n"], 4), "launches_per_step": b["n"],
         "method": "HIP events around each launch of one extra train step (in situ, launch stream)",
         # the same launches against the other roof: these passes sit under the 312 FLOP/B ridge
         "hbm": {"algorithmic_bytes_per_launch": round(b["b"] / b["n"]), "achieved": round(b["b"] / b["t"] / 1e6, 1),
                 "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(b["b"] / b["t"] / 1e6 / PEAK_HBM_GBS, 4)},
         "per_instance": {k: {"tflops": round(v["f"] / v["t"] / 1e9, 2), "ms_per_step": round(v["t"], 3), "launches": v["n"],
                              "avg_launch_ms": round(v["t"] / v["n"], 4),
                              "algorithmic_gbs": round(v["b"] / v["t"] / 1e6, 1)} for k, v in by.items()}}
    if src:
        r["traffic_source"] = ("profiles/" + src) if traffic else src
    fr = sustained_frontier()
    if fr and precision != "strict":
        # the matrix pipe and the HBM stream share one power budget: what the pipe sustains on real f16 operands next to a
        # stream of this kernel's measured (else algorithmic) HBM rate, by linear interpolation between the two measured arms
        alone, st, mx, fsrc = fr
        tbs = (traffic if traffic else b["b"] / b["n"]) / (b["t"] / b["n"]) / 1e9
        frontier = (alone - (alone - mx) / st * tbs) * 1e3
        executed = achieved * (3.0 if precision == "exact16" else 1.0)
        r["vs_sustained"] = {"matrix_alone_tflops": round(alone * 1e3, 1), "matrix_next_to_stream_tflops": round(mx * 1e3, 1),
                             "stream_tbs": st, "kernel_hbm_tbs": round(tbs, 2), "frontier_tflops": round(frontier, 1),
                             "executed_tflops": round(executed, 2), "frac": round(executed / frontier, 4),
                             "source": fsrc}
    return r


def roofline_from_probe(rows, precision):
    by = {}
    for r in rows:
        b = by.setdefault(r["kernel"], {"t": 0.0, "f": 0.0, "n": 0})
        b["t"] += r["ms"] * r["launches_per_step"]
        b["f"] += r["flop"] * r["launches_per_step"]
        b["n"] += r["launches_per_step"]
    name, b = max(by.items(), key=lambda kv: kv[1]["t"])
    achieved = b["f"] / b["t"] / 1e9
    peak = PEAK_F16_TFLOPS if precision == "fast" else PEAK_F32_TFLOPS
    return {"bound": "mfma", "kernel": name, "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": None,
            "avg_launch_ms": round(b["t"] / b["n"], 4), "launches_per_step": b["n"],
            "per_instance": {k: {"tflops": round(v["f"] / v["t"] / 1e9, 2), "ms_per_step": round(v["t"], 3),
                                 "launches": v["n"]} for k, v in by.items()}}


_CPU_BASELINE_SRC = r"""
import json, os, sys, time, random
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from oracle import model_ref as M
from oracle import degrade_ref as D
from oracle import imgproc_ref as I
threads = int(sys.argv[2]); probe_path = sys.argv[3]
torch.set_num_threads(threads)
out = {}

def mem_available_gb():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable"):
                return int(line.split()[1]) / 1048576.0
    except Exception:
        pass
    return 0.0

def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"

out["cpu_model"] = cpu_model()
# ---- parity probe: the oracle's forward on the probe the GPU modes were run on (weights and input from the parent) ----
if probe_path and os.path.exists(probe_path):
    pr = torch.load(probe_path, weights_only=False)
    with torch.no_grad():
        yo = M.generator_forward(pr["x"], pr["sd"], 4)
    out["probe"] = {k: float((v - yo).abs().max()) for k, v in pr["y"].items()}

sd = M.init_generator_state(0)
params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
opt = torch.optim.Adam(list(params.values()), 2e-4, (0.9, 0.99))
gen = torch.Generator().manual_seed(1234)

def gen_step(x, hr):
    t0 = time.time()
    opt.zero_grad(set_to_none=True)
    loss = (M.generator_forward(x, params, 4) - hr).abs().mean()
    loss.backward()
    opt.step()
    return time.time() - t0

# calibration on 64^2 (also warms the thread pool): the step is linear in pixels
x64 = torch.rand(1, 3, 64, 64, generator=gen); h64 = torch.rand(1, 3, 256, 256, generator=gen)
gen_step(x64, h64)
t64 = gen_step(x64, h64)
# the stated unit is one 256^2 -> 1024^2 image: run it when it fits the time / memory budget (autograd keeps ~20 GB of
# saved concatenations at this size), else 128^2 scaled x4
edge = 256 if (t64 * 16 < 45.0 and mem_available_gb() > 64.0) else 128
hr_edge = edge * 4
# degradation of ONE HR tile of the matching size through the oracle's loop-body restatement (train_realesrnet.py:262-377)
from real_esrgan_pytorch_amd_cfg import PROC_P, MODEL_P
random.seed(0); np.random.seed(0); torch.manual_seed(0)
base = torch.rand(1, 3, hr_edge // 16, hr_edge // 16, generator=gen)
hr = torch.nn.functional.interpolate(base, size=(hr_edge, hr_edge), mode="bicubic").clamp(0, 1)
hr = torch.round((0.9 * hr + 0.1 * torch.rand(1, 3, hr_edge, hr_edge, generator=gen)) * 255.0) / 255.0
k1, k2, ks = I.sample_sample_kernels(MODEL_P)
plan = D.sample_plan(hr_edge, hr_edge, hr_edge, PROC_P)
t0 = time.time()
with torch.no_grad():
    lr, hrc = D.degrade_batch(hr, torch.from_numpy(k1)[None].float(), torch.from_numpy(k2)[None].float(),
                              torch.from_numpy(ks)[None].float(), plan, PROC_P, 4, hr_edge)
t_deg = time.time() - t0
t_gen = gen_step(lr, hrc)
out.update({"edge": edge, "t64": t64, "t_degrade": t_deg, "t_generator": t_gen, "mem_available_gb": mem_available_gb()})
print(json.dumps(out))
"""


def cpu_baseline(probe_path="", timeout_s=240.0):
    """The CPU oracle (fp32 torch restatement of the reference, oracle/) on the host cores, on the stated unit of work:
    the second-order degradation of one HR tile (oracle/degrade_ref.py) + generator forward + backward + Adam on the
    resulting 256^2 -> 1024^2 pair (128^2 -> 512^2 scaled x4 when 256^2 does not fit the time / memory budget).  Runs in a
    child process with a hard timeout and a bounded thread count (an unbounded torch thread pool on a 256-thread host was
    ~700x slower than 8 threads).  The same child evaluates the oracle on the parity probe of the GPU modes."""
    import subprocess
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        avail = os.cpu_count() or 1
    threads = max(1, min(avail, 32))
    # the child needs the degradation parameter tables (plain dicts of the package's config.py) without importing the package
    # (which would load the HIP library): hand them over as a tiny generated module
    import tempfile
    from real_esrgan_pytorch_amd import config as cfg
    tmpdir = tempfile.mkdtemp(prefix="resr_cpu_baseline_")
    with open(os.path.join(tmpdir, "real_esrgan_pytorch_amd_cfg.py"), "w") as f:
        f.write("PROC_P = %r\nMODEL_P = %r\n" % (cfg.degradation_process_parameters_dict, cfg.degradation_model_parameters_dict))
    env = dict(os.environ, PYTHONPATH=tmpdir + os.pathsep + os.environ.get("PYTHONPATH", ""))
    try:
        r = subprocess.run([sys.executable, "-c", _CPU_BASELINE_SRC, ROOT, str(threads), probe_path],
                           capture_output=True, text=True, timeout=timeout_s, env=env)
        d = json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:
        return {"value": None, "unit": "images/sec", "cores": threads, "kind": "port",
                "sample": f"CPU oracle step did not finish within {timeout_s:.0f} s ({type(e).__name__})"}, None
    scale = (256 * 256) / float(d["edge"] * d["edge"])      # work is linear in pixels
    dt = (d["t_degrade"] + d["t_generator"]) * scale
    rec = {"value": round(1.0 / dt, 5), "unit": "images/sec", "cores": threads, "kind": "port", "cpu": d.get("cpu_model"),
           "sample": f"ONE image through the fp32 torch CPU oracle ({threads} threads of {avail} available): second-order degradation of a "
                     f"{d['edge'] * 4}^2 HR tile {d['t_degrade']:.2f} s + generator fwd+bwd+Adam {d['edge']}^2->{d['edge'] * 4}^2 "
                     f"{d['t_generator']:.2f} s" + ("" if scale == 1 else f", scaled x{scale:.0f} (linear in pixels) to the 256^2->1024^2 unit")
                     + f"; 64^2 calibration step {d['t64']:.2f} s"}
    return rec, d.get("probe")


def timed_region(fn, steps, world, sampler=None):
    """EXACTLY `steps` calls of fn bracketed by barrier + synchronize on both sides; seconds, the MAX over ranks."""
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    out = None
    t0 = time.perf_counter()
    if sampler is not None:
        with sampler:
            for _ in range(steps):
                out = fn()
            torch.cuda.synchronize()
    else:
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = tt.item()
    return dt, out


class LastCall:
    """--dump-outputs: keeps the input and output of a module's most recent forward (detached references, no copy and no
    synchronisation), so that what the last timed step fed and produced can be written after the timed region."""

    def __init__(self, module):
        self.x = self.y = self.out = None       # out: what the step itself returned (set by the step's caller)
        self._h = module.register_forward_hook(self._hook)

    def _hook(self, module, inputs, output):
        self.x, self.y = inputs[0].detach(), output.detach()

    def close(self):
        self._h.remove()


def dump_outputs(out_dir, arrays):
    """Write every tensor of `arrays` (None: skipped) as out_dir/<name>.npy in float32.  One of more than DUMP_SAMPLE elements is
    written as the flattened values at DUMP_SAMPLE sorted indices drawn from a fixed seed: the same arguments give the same indices."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        if t is None:
            continue
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randint(t.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.float().cpu().numpy())


def host_record(fn, world, reps=3):
    """What a step costs the HOST: wall time of issuing one step onto an idle device, no synchronisation inside (the launches
    are asynchronous, so this is Python + ctypes + runtime enqueue time, collectives' enqueue included).  A step whose enqueue
    time approaches ms_per_step is host-bound -- the first suspect when N ranks share a pod's CPUs.  Max / mean over ranks."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    mine = sorted(ts)[len(ts) // 2]
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 0)
    rec = {"enqueue_ms_per_step": round(mine, 2), "cpus_in_affinity": cpus, "cpus_online": os.cpu_count(),
           "how": f"median of {reps} steps issued onto an idle device, timed without a synchronisation"}
    try:
        rec["loadavg_1min"] = round(os.getloadavg()[0], 1)
    except OSError:
        pass
    if world > 1:
        t = torch.tensor([mine, -mine, float(cpus), -float(cpus)], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        s = torch.tensor([mine], device="cuda", dtype=torch.float64)
        dist.all_reduce(s, op=dist.ReduceOp.SUM)
        rec.update(enqueue_ms_per_step=round(t[0].item(), 2), enqueue_ms_min_rank=round(-t[1].item(), 2),
                   enqueue_ms_mean_rank=round(s.item() / world, 2), cpus_in_affinity=int(-t[3].item()),
                   cpus_in_affinity_max_rank=int(t[2].item()), note="enqueue_ms_per_step = MAX over ranks, cpus_in_affinity = MIN over ranks")
    return rec


def _emergency_line(args, world, steps, dt_seq, why):
    """The contract's JSON line from the SEQUENTIAL policy's timed steps alone -- printed by the watchdog of time_policies when the
    second policy (collectives overlapped with chained launches: a pairing no multi-GPU box has run before the first SCALE run)
    does not come back.  Minimal but valid: the driver gets its measurement whatever the experiment does."""
    B = args.batch
    lr_edge = args.lr_size
    value = B * world * steps / dt_seq
    gan = bool(args.gan)
    return {"metric": "x4 SR GAN train images/sec (RealESRGAN step, BASELINE config 4)" if gan else "x4 SR train images/sec (256->1024)",
            "value": round(value, 3), "unit": "images/sec", "n_gpus": world, "steps": steps, "warmup": args.warmup,
            "ms_per_step": round(dt_seq / steps * 1e3, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"fast": "f16", "exact16": "f16x2", "strict": "f32"}[args.precision], "data": "synthetic",
            "config": {"workload": ("RealESRGAN x4 GAN train step" if gan else "RealESRNet x4 L1 train step") + f", RRDBNet 23 blocks, LR {lr_edge}^2 -> HR {4 * lr_edge}^2, "
                                   f"batch {B}/GPU, degradation=hip", "global_batch": B * world, "parallelism": f"dp{world}"},
            "dist": {"world": world, "backend": dist.get_backend() if dist.is_initialized() else None,
                     "policies": {"sequential": {"ms_per_step": round(dt_seq / steps * 1e3, 2)}, "overlap_31cu": {"error": why}, "chosen": "sequential"}},
            "note": "emergency line: " + why}


def time_policies(args, steps, warmup, world, one, dp, model, dt_seq):
    """N > 1 (or a forced world-1 RCCL group): the gradient exchange has two policies and which one wins is a question only a
    multi-GPU box answers -- so the bench times BOTH in one process, K steps each on the same state:
      sequential    one all-reduce per arena, issued behind the backward pass (overlaps the next batch's degradation only);
      overlap_31cu  RESR_DP_OVERLAP=1: bucketed all-reduces on a communication stream behind the backward pass's range events,
                    with RESR_CHAIN_CUS_PER_XCD=31 (the chained launches leave one CU of every XCD to the collective).
    Returns (dt of the better policy, record); the model is left attached to the better policy."""
    if not dp.active:          # one rank, no process group: nothing is exchanged
        return dt_seq, None
    timed = {"ms_per_step": round(dt_seq / steps * 1e3, 2)}
    if getattr(dp, "overlap", False):   # the environment already selected the overlapped form: what was timed is not `sequential`
        return dt_seq, {"overlap_env": timed, "chosen": "overlap_env", "note": "RESR_DP_OVERLAP=1 in the environment: only that policy timed"}
    if args.single_policy:
        return dt_seq, {"sequential": timed, "chosen": "sequential", "note": "--single-policy: only the default policy timed"}
    rec = {"sequential": timed}
    prev_cus = os.environ.get("RESR_CHAIN_CUS_PER_XCD")
    os.environ["RESR_CHAIN_CUS_PER_XCD"] = "31"
    # Watchdog (every rank): the overlapped policy is an experiment; if it has not finished within 20 x what the sequential policy
    # took for the same steps (+ 60 s), rank 0 prints the sequential measurement as the contract's line and every rank leaves.
    import threading
    limit = 60.0 + 20.0 * dt_seq * (1 + max(1, min(warmup, 2)) / max(1, steps))
    rank = dist.get_rank() if dist.is_initialized() else 0

    def fire():
        why = f"the overlapped exchange policy did not finish within {limit:.0f} s: sequential policy reported"
        # The sequential measurement is complete and valid, so the contract's line is printed and the job leaves with
        # $RESR_BENCH_WATCHDOG_RC (default 0: "measurement valid"; the failed EXPERIMENT is in the line -- dist.policies.overlap_31cu.error,
        # `note` -- and on every rank's stderr).  A non-zero code here would make the launcher discard a good line.
        sys.stderr.write(f"bench.py rank {rank}: WATCHDOG -- {why}\n")
        sys.stderr.flush()
        if rank == 0:
            print(json.dumps(_emergency_line(args, world, steps, dt_seq, why)), flush=True)
        os._exit(int(os.environ.get("RESR_BENCH_WATCHDOG_RC", "0")))
    wd = threading.Timer(limit, fire)
    wd.daemon = True
    wd.start()
    import real_esrgan_pytorch_amd as _R
    errs_before = int(_R._lib.lib().resr_debug_chain_errors())
    try:
        model.grad_hook = None
        dp.attach(model, overlap=True)
        for _ in range(max(1, min(warmup, 2))):
            one()
        dt_ov, _ = timed_region(one, steps, world)
    finally:
        wd.cancel()
    rec["overlap_31cu"] = {"ms_per_step": round(dt_ov / steps * 1e3, 2)}
    errs_after = int(_R._lib.lib().resr_debug_chain_errors())
    if errs_after != errs_before:    # a chained launch gave up on a neighbour next to the collective: never the policy to report
        rec["overlap_31cu"]["chain_errors"] = errs_after - errs_before
        rec["overlap_31cu"]["note"] = "chained launches timed out next to the overlapped collectives (their outputs are NaN-poisoned): policy rejected"
        dt_ov = float("inf")
    if dt_ov < dt_seq:
        rec["chosen"] = "overlap_31cu"
        return dt_ov, rec
    rec["chosen"] = "sequential"
    if prev_cus is None:
        os.environ.pop("RESR_CHAIN_CUS_PER_XCD", None)
    else:
        os.environ["RESR_CHAIN_CUS_PER_XCD"] = prev_cus
    model.grad_ready_hook = None
    dp.attach(model, overlap=False)
    return dt_seq, rec


def make_hr_tiles(args, B, hr_edge, rank):
    g = torch.Generator(device="cuda").manual_seed(1234 + rank)
    hr = torch.round(torch.rand(B, 3, hr_edge, hr_edge, device="cuda", generator=g) * 255.0) / 255.0
    if not args.noise_data:   # image-like tiles (bicubic-upsampled noise + grain): keeps the output off the clamp, so the backward
        # pass carries dense gradients (on uniform-noise tiles the first Adam step saturates the clamp, model.py:270)
        base = torch.rand(B, 3, hr_edge // 16, hr_edge // 16, device="cuda", generator=g)
        hr = torch.nn.functional.interpolate(base, size=(hr_edge, hr_edge), mode="bicubic").clamp(0, 1)
        hr = torch.round((0.9 * hr + 0.1 * torch.rand(B, 3, hr_edge, hr_edge, device="cuda", generator=g)) * 255.0) / 255.0
    return hr


def run_mode(args, precision, steps, warmup, world, rank, probe=True, centre_output=False, degradation_record=False, dump_dir=None):
    """Build the training state in `precision`, run `warmup` untimed + `steps` timed steps (barrier + synchronize on both
    sides, max over ranks), optionally write what the last of them computed (dump_dir) and, with --full, one more step with
    per-launch events for the roofline record."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.train import DataParallel, RealESRNetStep

    torch.manual_seed(0)                                  # reference config.py:64-66: same init on every rank
    model = R.Generator(3, 3, 4, precision=precision).cuda()
    model.train()
    if centre_output:   # start the output in the middle of the training-time clamp (model.py:270) instead of around 0
        with torch.no_grad():
            model.conv4.bias.add_(0.5)
    torch.cuda.manual_seed(1234 + rank)                   # device-side draws of the degradation (sigma, quality, ...) differ per rank
    dp = DataParallel()
    dp.attach(model)
    ema = R.EMA(model, 0.999)                             # config.py:102
    ema.register()
    # config.py:100-101.  Default: Adam over the one Parameter that aliases the flat arena (same update, one launch);
    # --per-tensor-adam: over the 702 per-tensor Parameters like the reference's script
    opt_params = model.parameters() if args.per_tensor_adam else [model.flat_parameter()]
    opt = torch.optim.Adam(opt_params, 2e-4, (0.9, 0.99), fused=True)
    scaler = torch.amp.GradScaler("cuda") if precision != "strict" else None  # train_realesrnet.py:97

    B, lr_edge = args.batch, args.lr_size
    hr_edge = lr_edge * 4
    hr = make_hr_tiles(args, B, hr_edge, rank)
    degrade = None
    degradation = "none"
    if not args.no_degradation:
        from real_esrgan_pytorch_amd.degrade import Degrader
        degrade = Degrader(batch=B, hr_size=hr_edge, upscale=4, crop=hr_edge, seed=rank)
        degradation = "hip"
    lr_fixed = None
    if degrade is None:
        lr_fixed = torch.nn.functional.interpolate(hr, scale_factor=0.25, mode="area")
    step = RealESRNetStep(model, ema, opt, scaler, degrade)
    cap = LastCall(model) if dump_dir and rank == 0 else None

    def one():
        out = step(hr, lr_fixed)
        if cap is not None:
            cap.out = out
        return out

    for _ in range(warmup):
        one()
    sampler = PowerSampler() if args.full else None
    dt, loss = timed_region(one, steps, world, sampler)
    dt, policies = time_policies(args, steps, warmup, world, one, dp, model, dt)
    res = {"precision": precision, "dt": dt, "steps": steps, "warmup": warmup, "loss": float(loss), "degradation": degradation,
           "policies": policies}
    if cap is not None:     # before any further step changes the state
        cap.close()
        dump_outputs(dump_dir, {"loss": cap.out, "lr": cap.x, "sr": cap.y, "params": model.flat_parameters(), "grad": model.flat_grad(),
                                "ema": torch.cat([ema.shadow[n].reshape(-1) for n, _ in model.named_parameters()])})
    if args.full:
        res.update(power=sampler.summary(), host=host_record(one, world))

    # The in-situ roofline probe is one more (untimed) train step.  With several ranks that step contains the gradient
    # all-reduce, so every rank runs it; only rank 0 brackets its launches with events and reports.  A failure on any rank
    # is agreed on by all ranks (no rank may skip a collective the others are in).
    if probe and not args.no_probe:
        err = None
        try:
            if rank == 0:
                res["roofline"] = roofline_in_situ(one, precision, B)
            else:
                one()
                torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            err = repr(e)
        if world > 1:
            ok = torch.tensor([0 if err is None else 1], device="cuda")
            dist.all_reduce(ok)
            if int(ok.item()):
                dist.destroy_process_group()
                raise SystemExit(f"roofline probe step failed on a rank: {err}")
        elif err is not None:
            res["roofline"] = {"error": err}

    if degradation_record and rank == 0 and world == 1 and degrade is not None and not args.no_probe:
        # the degradation stage against its own (HBM) roofline + what it costs the step: a few more steps fed pre-degraded tiles
        try:
            lr_pre, hr_pre = degrade(hr)
            lr_pre, hr_pre = lr_pre.clone(), hr_pre.clone()
            torch.cuda.synchronize()
            k = max(3, min(steps, 8))
            step(hr_pre, lr_pre)
            dt0, _ = timed_region(lambda: step(hr_pre, lr_pre), k, 1)
            res["degradation_roofline"] = degradation_roofline(degrade, hr, B, dt / steps * 1e3, dt0 / k * 1e3)
            del lr_pre, hr_pre
        except Exception as e:  # pragma: no cover
            res["degradation_roofline"] = {"error": repr(e)}

    if rank == 0 and args.full:
        with torch.no_grad():
            sr_probe = model(torch.nn.functional.interpolate(hr[:2], scale_factor=0.25, mode="area"))
            res["unclamped"] = round(float(((sr_probe > 0) & (sr_probe < 1)).float().mean()), 4)
            del sr_probe
        res["state_dict"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    del step, degrade, opt, ema, dp, model, hr
    torch.cuda.empty_cache()
    return res


D_MAC_PER_HR_PX = 395_520          # discriminator forward MACs per input pixel (SURVEY.md §8 geometry)


def run_gan(args, world, rank, dump_dir=None):
    """BASELINE config 4, this rank's share: one RealESRGAN optimisation step per `step` on synthetic HR tiles resident in
    HBM.  Data parallel: generator gradients from its backward hook, discriminator gradients once after the second backward."""
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.degrade import Degrader
    from real_esrgan_pytorch_amd.train import DataParallel, RealESRGANStep

    torch.manual_seed(0)
    g = R.Generator(3, 3, 4, precision=args.precision).cuda().train()
    d = R.Discriminator(precision=args.precision).cuda().train()
    torch.cuda.manual_seed(1234 + rank)
    dp = DataParallel()
    dp.attach(g)
    dp.attach_discriminator(d)
    ema = R.EMA(g, 0.999)
    ema.register()
    g_opt = torch.optim.Adam(g.parameters() if args.per_tensor_adam else [g.flat_parameter()], 1e-4, (0.9, 0.99), fused=True)   # config.py:141-142
    d_opt = torch.optim.Adam(d.parameters() if args.per_tensor_adam else [d.flat_parameter()], 1e-4, (0.9, 0.99), fused=True)
    content = R.ContentLoss(["features.2", "features.7", "features.16", "features.25", "features.34"], [0.485, 0.456, 0.406],
                            [0.229, 0.224, 0.225], precision=args.precision).cuda()
    B = args.batch
    crop = args.lr_size * 4
    tile = 400 if crop == 256 else crop              # reference tiles are 400^2, cropped to config.image_size (scripts/run.py:17)
    hr = make_hr_tiles(args, B, tile if tile % 16 == 0 else crop, rank)
    if hr.shape[-1] != tile:
        hr = torch.nn.functional.interpolate(hr, size=(tile, tile), mode="bilinear").clamp(0, 1)
        hr = torch.round(hr * 255.0) / 255.0
    degrade = Degrader(batch=B, hr_size=tile, upscale=4, crop=crop, seed=rank)
    scaler = torch.amp.GradScaler("cuda") if args.precision != "strict" else None
    step = RealESRGANStep(g, d, ema, g_opt, d_opt, scaler, degrade, content_criterion=content, dp=dp)
    cap = LastCall(g) if dump_dir and rank == 0 else None

    def one():
        out = step(hr)
        if cap is not None:
            cap.out = out
        return out

    for _ in range(args.warmup):
        out = one()
    dt, out = timed_region(one, args.steps, world)
    dt, policies = time_policies(args, args.steps, args.warmup, world, one, dp, g, dt)
    res = {"dt": dt, "losses": {k: round(float(v), 6) for k, v in out.items()}, "tile": tile, "crop": crop, "policies": policies}
    if cap is not None:     # before any further step changes the state
        cap.close()
        dump_outputs(dump_dir, {**cap.out, "lr": cap.x, "sr": cap.y, "g_params": g.flat_parameters(),
                                "d_params": d.flat_parameters(), "ema": torch.cat([ema.shadow[n].reshape(-1) for n, _ in g.named_parameters()])})
    if args.full:
        res["host"] = host_record(one, world)
    if not args.no_probe:
        err = None
        try:
            if rank == 0:
                res["roofline"] = roofline_in_situ(lambda: step(hr), args.precision, B)
            else:
                step(hr)
                torch.cuda.synchronize()
        except Exception as e:  # pragma: no cover
            err = repr(e)
        if world > 1:
            ok = torch.tensor([0 if err is None else 1], device="cuda")
            dist.all_reduce(ok)
            if int(ok.item()):
                dist.destroy_process_group()
                raise SystemExit(f"roofline probe step failed on a rank: {err}")
        elif err is not None:
            res["roofline"] = {"error": err}
    return res


def gan_main(args, world, rank):
    res = run_gan(args, world, rank, dump_dir=args.dump_outputs)
    res["devices"] = gather_devices(world, rank)     # a collective: every rank
    if rank != 0:
        return
    B, crop = args.batch, res["crop"]
    value = B * world * args.steps / res["dt"]
    lr_edge = crop // 4
    # algorithmic FLOP per image: generator train step 3 x forward; discriminator 3 fwd + 3 dgrad + 2 wgrad = 8 forward-equivalents
    flop_g = 3 * 2 * MAC_PER_LR_PX * lr_edge * lr_edge
    flop_d = 16 * D_MAC_PER_HR_PX * crop * crop
    out = {
        "metric": "x4 SR GAN train images/sec (RealESRGAN step, BASELINE config 4)", "value": round(value, 3), "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(res["dt"] / args.steps * 1e3, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": {"fast": "f16", "exact16": "f16x2 (split-operand f16 MFMA: generator, discriminator and VGG19)", "strict": "f32"}[args.precision], "data": "synthetic",
        "data_detail": "uniform-noise HR tiles" if args.noise_data else "image-like HR tiles (bicubic-upsampled noise + 10 % grain, quantised to k/255)",
        "config": {"workload": f"RealESRGAN x4 GAN train step (G update with D frozen + USM(sr) + VGG19 term, then D(hr) / D(sr) backwards), "
                               f"RRDBNet 23 blocks + SN U-Net discriminator, HR tiles {res['tile']}^2 cropped to {crop}^2 (LR {lr_edge}^2), "
                               f"batch {B}/GPU, degradation=hip, 2 x Adam + EMA, shared GradScaler",
                   "global_batch": B * world, "parallelism": f"dp{world}"},
        "algorithmic_tflops_per_gpu": round(value / world * (flop_g + flop_d) / 1e12, 2),
        "losses": res["losses"],
        "chain_errors": int(__import__("real_esrgan_pytorch_amd")._lib.lib().resr_debug_chain_errors()),
        "dist": dist_record(world, res.get("devices"), res.get("policies")),
    }
    for k in ("host", "roofline"):     # --full
        if k in res:
            out[k] = res[k]
    print(json.dumps(out), flush=True)


def compact_roofline(r):
    """Dominant instance of a probed step for the other_configs records."""
    if not r or "error" in r:
        return r
    return {"kernel": r["kernel"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"],
            "avg_launch_ms": r["avg_launch_ms"], "launches_per_step": r["launches_per_step"],
            "per_instance": {k: {"tflops": v["tflops"], "ms_per_step": v["ms_per_step"], "launches": v["launches"]} for k, v in r["per_instance"].items()}}


def gather_devices(world, rank):
    """Which GPU every rank drives (a collective when world > 1: call it on every rank).  `distinct` < world means ranks share
    a device -- the single-GPU control-flow tests do, a SCALE run must not."""
    dev = torch.cuda.current_device()
    props = torch.cuda.get_device_properties(dev)
    mine = {"rank": rank, "local_index": dev, "name": props.name, "uuid": str(getattr(props, "uuid", "")),
            "pci": "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0), getattr(props, "pci_device_id", 0)),
            "cus": props.multi_processor_count, "hbm_gb": round(props.total_memory / 2 ** 30, 1),
            "visible": os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES") or os.environ.get("CUDA_VISIBLE_DEVICES")}
    allv = [mine]
    if world > 1:
        allv = [None] * world
        dist.all_gather_object(allv, mine)
    ids = {(d["uuid"], d["pci"]) if (d["uuid"] or d["pci"] != "0000:00:00") else ("rank-local", d["local_index"], d["visible"]) for d in allv}
    return {"count": len(allv), "distinct": len(ids), "per_rank": allv}


def dist_record(world, devices=None, policies=None):
    """What the collective layer saw: a SCALE line must show that RCCL ran with N ranks on N distinct GPUs."""
    rec = {"world": world, "backend": dist.get_backend() if dist.is_initialized() else None,
           "nranks": dist.get_world_size() if dist.is_initialized() else 1,
           "overlap_with_backward": os.environ.get("RESR_DP_OVERLAP", "0") == "1",
           "forced_collectives": os.environ.get("RESR_DP_FORCE", "0") == "1"}
    if devices is not None:
        rec["devices"] = devices["distinct"]
        rec["device_list"] = devices["per_rank"]
        if devices["distinct"] < world:
            rec["warning"] = f"{world} ranks on {devices['distinct']} distinct device(s): ranks SHARE a GPU (control-flow test, not a scaling measurement)"
    if policies is not None:
        rec["policies"] = policies
    try:
        v = torch.cuda.nccl.version()
        rec["rccl_version"] = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    except Exception:
        rec["rccl_version"] = None
    return rec


def other_configs(args):
    """Short runs of the other BASELINE.json configurations on this GPU (N = 1 only), so that every configuration has a number
    from the same driver-run process as the headline.  They are parity-test cases (tests/), not the headline metric."""
    import copy
    import real_esrgan_pytorch_amd as R
    from real_esrgan_pytorch_amd.tiling import TiledGenerator
    out = {}

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    try:    # config 2: RRDBNet x4 f16 inference, batch 16 of 256^2 LR (generator kernels only)
        torch.manual_seed(0)
        g4 = R.Generator(3, 3, 4, precision="fast").cuda().eval()
        x = torch.rand(16, 3, 256, 256, device="cuda")
        with torch.no_grad():
            dt = timed(lambda: g4(x), 5)
        flop = 2 * MAC_PER_LR_PX * 256 * 256 * 16
        rec2 = {"images_per_sec": round(16 / dt, 1), "ms": round(dt * 1e3, 2),
                "tflops": round(flop / dt / 1e12, 1), "frac_of_f16_peak": round(flop / dt / 1e12 / PEAK_F16_TFLOPS, 3)}
        sd2 = g4.state_dict()
        del g4
        torch.cuda.empty_cache()
        # the same batch in the mode inference.py / test.py default to (the reference runs these call sites in fp32)
        g4x = R.Generator(3, 3, 4, precision="exact16")
        g4x.load_state_dict(sd2)
        g4x = g4x.cuda().eval()
        with torch.no_grad():
            dtx = timed(lambda: g4x(x), 3)
        rec2["parity_mode"] = {"precision": "exact16 (the default of inference.py / test.py: fp32 call sites of the reference); inference plan (x2_plan bits 0, 5, 6): residual "
                                            "stream and HR tail as pairs on ONE f16 stage + ONE MX stage (both 2^-12-weighted corrections as v_mfma_scale_f32_32x32x64_f8f6f4 on "
                                            "unscaled bf8 records), growth planes single f16 against f16 weights -- 30 stage-equivalents per dense block instead of 60; forward "
                                            "0.9-1.14e-4 vs the fp32 oracle at init scale / dense weights x 4, 6e-5 on trained weights (gate 2e-4, tests/test_gpu_mx.py)",
                               "x2_plan_effective": int(g4x.x2_plan),
                               "images_per_sec": round(16 / dtx, 1), "ms": round(dtx * 1e3, 2), "tflops_algorithmic": round(flop / dtx / 1e12, 1)}
        # ... and round 5's plan behind the knob (x2_plan = 59: three f16 stages per pair chunk, 40 stages per block; forward 2.3e-6 / 2.9e-5)
        del g4x
        torch.cuda.empty_cache()
        g4y = R.Generator(3, 3, 4, precision="exact16", x2_plan=59)
        g4y.load_state_dict(sd2)
        g4y = g4y.cuda().eval()
        with torch.no_grad():
            dty = timed(lambda: g4y(x), 3)
        rec2["parity_mode"]["without_mx_stages"] = {"knob": "x2_plan=59 / RESR_X2_PLAN=59 (round 5's default: forward 2.3e-6 / 2.9e-5)", "images_per_sec": round(16 / dty, 1),
                                                    "ms": round(dty * 1e3, 2)}
        out["config2_x4_f16_inference_b16_lr256"] = rec2
        del g4y, x, sd2
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        out["config2_x4_f16_inference_b16_lr256"] = {"error": repr(e)}
    try:    # config 3: RealESRNet x4 L1 training, batch 32 of 256^2 HR tiles (LR 64^2), degradation on the side stream
        a3 = copy.copy(args)
        a3.batch, a3.lr_size, a3.no_probe = 32, 64, False
        # random init puts the output around 0; at this size a first Adam step that overshoots the clamp leaves the step with
        # zero gradients for good (loss 0.4998, 8 % "faster"): centre the output bias so the timed regime carries real gradients
        r = run_mode(a3, "fast", 20, 5, 1, 0, probe=True, centre_output=True)
        v = 32 * r["steps"] / r["dt"]
        out["config3_realesrnet_train_b32_hr256"] = {"images_per_sec": round(v, 1), "ms_per_step": round(r["dt"] / r["steps"] * 1e3, 2),
                                                     "tflops": round(v * 3 * 2 * MAC_PER_LR_PX * 64 * 64 / 1e12, 1),
                                                     "frac_of_f16_peak": round(v * 3 * 2 * MAC_PER_LR_PX * 64 * 64 / 1e12 / PEAK_F16_TFLOPS, 3),
                                                     "loss": r["loss"], "unclamped_output_fraction": r.get("unclamped"),
                                                     "init": "reference init, conv4.bias + 0.5 (output starts inside the training-time clamp)",
                                                     "power": r.get("power"),
                                                     "roofline": compact_roofline(r.get("roofline"))}
        del r
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        out["config3_realesrnet_train_b32_hr256"] = {"error": repr(e)}
    try:    # config 4, this GPU's share: RealESRGAN step, batch 16, HR 400^2 tiles cropped to 256^2 (full record: bench.py --gan)
        a4 = copy.copy(args)
        a4.batch, a4.lr_size, a4.no_probe, a4.steps, a4.warmup, a4.precision = 16, 64, False, 20, 8, "fast"   # (the degradation's per-batch sizes keep the caching allocator growing for a few steps: 3 warm-up steps left hipMallocs inside 10 timed ones)
        r = run_gan(a4, 1, 0)
        rec = {"images_per_sec": round(16 * a4.steps / r["dt"], 1), "ms_per_step": round(r["dt"] / a4.steps * 1e3, 2), "losses": r["losses"],
               "roofline": compact_roofline(r.get("roofline"))}
        del r
        torch.cuda.empty_cache()
        # the same step in the mode that meets the 1e-3 tolerance: generator, discriminator AND VGG19 on split-operand f16 MFMA
        a4.precision, a4.steps, a4.warmup, a4.no_probe = "exact16", 10, 4, True
        r = run_gan(a4, 1, 0)
        rec["parity_mode"] = {"precision": "exact16 (generator, discriminator and VGG19 on hi/lo f16 pairs)",
                              "images_per_sec": round(16 * a4.steps / r["dt"], 1), "ms_per_step": round(r["dt"] / a4.steps * 1e3, 2),
                              "losses": r["losses"]}
        out["config4_realesrgan_step_b16_hr256_per_gpu"] = rec
        del r
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        out["config4_realesrgan_step_b16_hr256_per_gpu"] = {"error": repr(e)}
    try:    # the headline geometry at the reference's own batch_size (48 per process, config.py:90)
        a48 = copy.copy(args)
        a48.batch, a48.lr_size, a48.no_probe = 48, 256, True
        r = run_mode(a48, "fast", 5, 2, 1, 0, probe=False)
        v = 48 * r["steps"] / r["dt"]
        out["reference_batch48_lr256"] = {"images_per_sec": round(v, 1), "ms_per_step": round(r["dt"] / r["steps"] * 1e3, 2),
                                          "tflops": round(v * 3 * 2 * MAC_PER_LR_PX * 256 * 256 / 1e12, 1),
                                          "frac_of_f16_peak": round(v * 3 * 2 * MAC_PER_LR_PX * 256 * 256 / 1e12 / PEAK_F16_TFLOPS, 3),
                                          "loss": r["loss"], "power": r.get("power")}
        del r
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        out["reference_batch48_lr256"] = {"error": repr(e)}
    try:    # config 5: RRDBNet x2, 3840x2160 LR frame, tiled, whole-frame hipGraph
        torch.manual_seed(0)
        g2 = R.Generator(3, 3, 2, precision="fast").cuda().eval()
        frame = torch.rand(1, 3, 2160, 3840, device="cuda")
        from real_esrgan_pytorch_amd.tiling import DEFAULT_HALO
        tg = TiledGenerator(g2, halo=DEFAULT_HALO, use_graph=True)      # the halo inference.py / test.py tile with (64; rounds 2-5 timed halo 32)
        tiles, wh, ww = tg.plan(1, 2160, 3840)
        dt = timed(lambda: tg(frame), 3)
        flop = 2 * 17_932_032 * 1920 * 1080
        out["config5_x2_4k_tiled_hipgraph"] = {"frames_per_sec": round(1 / dt, 3), "ms": round(dt * 1e3, 1), "tflops": round(flop / dt / 1e12, 1),
                                               "frac_of_f16_peak": round(flop / dt / 1e12 / PEAK_F16_TFLOPS, 3),
                                               "tiles": len(tiles), "window": [wh, ww], "halo": DEFAULT_HALO}
        try:    # ... and at the halo the rounds before measured (32), for continuity with their numbers
            tg32 = TiledGenerator(g2, halo=32, use_graph=True)
            dt32 = timed(lambda: tg32(frame), 2)
            out["config5_x2_4k_tiled_hipgraph"]["halo32"] = {"frames_per_sec": round(1 / dt32, 3), "ms": round(dt32 * 1e3, 1)}
            del tg32
        except Exception as e:  # pragma: no cover
            out["config5_x2_4k_tiled_hipgraph"]["halo32"] = {"error": repr(e)}
        del g2, frame, tg
        torch.cuda.empty_cache()
    except Exception as e:  # pragma: no cover
        out["config5_x2_4k_tiled_hipgraph"] = {"error": repr(e)}
    return out


def parity_probe(sd, edge=24):
    """Max-abs distance of every precision mode's forward to the strict (f32 MFMA) one on a seeded edge x edge probe with the
    timed model's weights; nothing from oracle/ is involved here (the CPU oracle's view of the same probe is added by the
    cpu_baseline leg)."""
    import real_esrgan_pytorch_amd as R
    x = torch.rand(1, 3, edge, edge, generator=torch.Generator().manual_seed(99)).cuda()
    ys = {}
    for precision in ("strict", "exact16", "fast"):
        g = R.Generator(3, 3, 4, precision=precision)
        g.load_state_dict(sd)
        g = g.cuda().eval()
        with torch.no_grad():
            ys[precision] = g(x).float().cpu()
        del g
    torch.cuda.empty_cache()
    return x.cpu(), ys


def gradient_probe(sd, batch, lr_edge):
    """What training consumes: every gradient tensor of the benchmarked f16 mode (and of exact16's default plan) against exact16's
    all-pairs plan (5.8e-6 from float64 where the emulation reaches) -- same weights (the timed model's, after its steps), same image-like
    batch at the benchmark's geometry, the train step's L1 mean loss at a GradScaler's initial scale.  Per-tensor relative L2."""
    import real_esrgan_pytorch_amd as R
    gen = torch.Generator(device="cuda").manual_seed(77)
    hr_edge = 4 * lr_edge
    base = torch.rand(batch, 3, hr_edge // 16, hr_edge // 16, device="cuda", generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(hr_edge, hr_edge), mode="bicubic").clamp(0, 1)
    hr = (0.9 * hr + 0.1 * torch.rand(batch, 3, hr_edge, hr_edge, device="cuda", generator=gen)).clamp(0, 1)
    lr = torch.nn.functional.interpolate(hr, size=(lr_edge, lr_edge), mode="area")

    def grads(precision, plan):
        g = R.Generator(3, 3, 4, precision=precision, x2_plan=plan)
        g.load_state_dict(sd)
        g = g.cuda().train()
        ((g(lr) - hr).abs().mean() * 65536.0).backward()
        torch.cuda.synchronize()
        out = {n: p.grad.detach().double() / 65536.0 for n, p in g.named_parameters()}
        del g
        torch.cuda.empty_cache()
        return out
    ref = grads("exact16", 0)
    rec = {"loss": "mean |G(lr) - hr| x 65536 (a GradScaler's initial scale)", "geometry": f"{batch} x 3 x {lr_edge}^2 -> {hr_edge}^2, image-like tiles",
           "reference": "exact16, all-pairs plan (x2_plan = 0), same weights and batch", "metric": "relative L2 per gradient tensor (702 tensors)"}
    for name, (precision, plan) in {"fast_f16": ("fast", 0), "exact16_default_plan": ("exact16", None)}.items():
        got = grads(precision, plan)
        rel = sorted(((got[k] - ref[k]).norm() / ref[k].norm().clamp_min(1e-300)).item() for k in ref)
        rec[name] = {"median": float(f"{rel[len(rel) // 2]:.3e}"), "p90": float(f"{rel[int(len(rel) * 0.9)]:.3e}"), "worst": float(f"{rel[-1]:.3e}")}
    return rec


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args.gpus))      # plain `python bench.py --gpus N`: this process never touches the GPU
    if args.gpus != world:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node and --gpus disagree")
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X: the hot path has no CPU fallback")
    dev_index = local_rank % torch.cuda.device_count()   # one rank per GPU; wraps only in the single-GPU control-flow test
    torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes)
        backend = os.environ.get("RESR_BENCH_BACKEND", "nccl")     # "gloo": ranks sharing one GPU (tests/test_gpu_dp.py)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    elif os.environ.get("RESR_BENCH_FORCE_NCCL", "0") == "1":
        # One GPU, but the RCCL path for real: a world-1 `nccl` group launches genuine RCCL kernels (ReduceOp.AVG on arena slices,
        # the communication stream, RCCL next to chained conv launches) -- the collective code a SCALE run uses, minus the peers.
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(so.getsockname()[1])
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ["RESR_DP_FORCE"] = "1"
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", dev_index))
    if rank == 0:
        ensure_built()
    if world > 1:
        dist.barrier()
    if rank == 0 and not args.no_probe and not args.no_sustained and args.precision != "strict":
        measure_sustained_frontier()         # this box's power-cap frontier (~3 s), before the timed steps

    if args.gan:
        gan_main(args, world, rank)
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    B, lr_edge = args.batch, args.lr_size
    hr_edge = lr_edge * 4
    main_res = run_mode(args, args.precision, args.steps, args.warmup, world, rank, centre_output=args.centre_output, degradation_record=True,
                        dump_dir=args.dump_outputs)
    devices = gather_devices(world, rank)      # a collective: every rank
    # the mode that meets north_star's 1e-3 tolerance, timed on the same workload (fewer steps: it is ~2.5x slower)
    parity_res = parity_hi = parity_p7 = None
    if args.precision == "fast" and not args.no_parity_mode:
        parity_res = run_mode(args, "exact16", max(2, min(args.steps, 8)), min(args.warmup, 2), world, rank, probe=True)
        # ... and with the opt-in hi-tensors-only weight gradients (RESR_X2_WGRAD_PRODUCTS=1: a third of their matrix work, every
        # gradient tensor 3-9e-4 from the float64 evaluation instead of 6e-6 -- inside 1e-3 without real margin, hence opt-in)
        os.environ["RESR_X2_WGRAD_PRODUCTS"] = "1"
        try:
            parity_hi = run_mode(args, "exact16", max(2, min(args.steps, 4)), 1, world, rank, probe=False)
        finally:
            os.environ.pop("RESR_X2_WGRAD_PRODUCTS", None)
        # ... and round 5's default plan (x2_plan = 59: without the MX stages of the backward-data passes) behind its knob
        prev_plan = os.environ.get("RESR_X2_PLAN")
        os.environ["RESR_X2_PLAN"] = "59"
        try:
            parity_p7 = run_mode(args, "exact16", max(2, min(args.steps, 4)), 1, world, rank, probe=False)
        finally:
            if prev_plan is None:
                os.environ.pop("RESR_X2_PLAN", None)
            else:
                os.environ["RESR_X2_PLAN"] = prev_plan

    if rank == 0:
        flop_per_image = 3 * 2 * MAC_PER_LR_PX * lr_edge * lr_edge

        def rate(res):
            return B * world * res["steps"] / res["dt"]
        value = rate(main_res)
        out = {
            "metric": "x4 SR train images/sec (256->1024)", "value": round(value, 3), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(main_res["dt"] / args.steps * 1e3, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"fast": "f16", "exact16": "f16x2 (split-operand f16 MFMA, fp32 accumulate)", "strict": "f32"}[args.precision], "data": "synthetic",
            "data_detail": "uniform-noise HR tiles" if args.noise_data else "image-like HR tiles (bicubic-upsampled noise + 10 % grain, quantised to k/255)",
            "config": {"workload": f"RealESRNet x4 L1 train step, RRDBNet 23 blocks, LR {lr_edge}^2 -> HR {hr_edge}^2, "
                                   f"batch {B}/GPU, degradation={main_res['degradation']}, Adam+EMA, GradScaler",
                       "global_batch": B * world, "parallelism": f"dp{world}"},
            "generator_tflops_per_gpu": round(value / world * flop_per_image / 1e12, 2),
            "loss": main_res["loss"],
            # chained dense-block launches: polls that timed out + workgroups beyond an XCD's share (resr_debug_chain_errors); must be 0
            "chain_errors": int(__import__("real_esrgan_pytorch_amd")._lib.lib().resr_debug_chain_errors()),
            "dist": dist_record(world, devices, main_res.get("policies")),
        }
        if args.full:
            # health of the timed regime: the share of output values strictly inside the training-time clamp (model.py:270).
            # Near 0 the backward pass multiplies (almost) only zeros and runs faster than on real gradients (see --noise-data)
            out["unclamped_output_fraction"] = main_res.get("unclamped")
            # rank 0's board power / shader clock over the timed steps (the step runs at the power cap: DESIGN section 5)
            out["power"] = main_res.get("power")
            # host side of a step (enqueue time without a sync, CPUs this process may run on): max over ranks
            out["host"] = main_res.get("host")
        if "roofline" in main_res:
            out["roofline"] = main_res["roofline"]
            if "degradation_roofline" in main_res and isinstance(out["roofline"], dict):
                out["roofline"]["degradation"] = main_res["degradation_roofline"]
            pw = main_res.get("power")
            if pw and pw.get("sclk_mhz_avg") and precision_is_f16(main_res):
                # the contract's frac stays priced against the nominal peak (2.4 GHz); next to it, the same rate against what the
                # matrix pipe can issue at the shader clock the power cap left it during the timed steps
                pk = PEAK_F16_TFLOPS * pw["sclk_mhz_avg"] / 2400.0
                out["roofline"]["at_measured_clock"] = {"sclk_mhz": pw["sclk_mhz_avg"], "peak": round(pk, 1),
                                                         "frac": round(out["roofline"]["achieved"] / pk, 4)}
        probe_path, probe_err = "", None
        if parity_res is not None:
            pv = rate(parity_res)
            pm = {"precision": "exact16",
                  "what": "the same train step with split-operand f16 MFMA (activations and weights as hi+lo f16 pairs, three MFMAs per "
                          "product, fp32 accumulate): the mode that meets the 1e-3 max-abs parity tolerance vs the fp32 CPU path",
                  "x2_plan_effective": int(os.environ.get("RESR_X2_PLAN", "763")),
                  "x2_plan": "default (763; its training bits 27 + 128 + 512): forward all pairs; the dense blocks' backward-data passes read EVERY gradient chunk as a pair on one f16 + "
                             "one MX stage (round 6: unscaled bf8 q records from the producing epilogues; 40 stage-equivalents per block); their weight gradients take both "
                             "2^-12-weighted tap-products of every stream chunk as ONE MX job (8-bit transpose reads, K = 32 pixels twice per v_mfma_scale_f32_32x32x64_f8f6f4) -- "
                             "worst gradient tensor 5.6-6.5e-5 against the all-pairs plan on the GPU (round 5's plan 27: 2.2-2.6e-4); for the growth chunks round 5's plan stays: "
                             "conv1..conv4's products read G's hi tensor and the weight products read "
                             "the growth planes as their hi tensor, conv5's such products with g_y's hi tensor (46 instead of 78 tap-products per dense block; worst gradient tensor "
                             "2.2-4.6e-4 vs float64 in the emulation at three geometries x five seeds; against the all-pairs plan on the GPU at 16 x 256^2 .. "
                             "1 x 24^2: 1.7-5.1e-4 under a dense random cotangent, 5e-7 .. 2e-5 under this step's L1 loss -- profiles/r05_x2_plan_validate.json, "
                             "DESIGN section 2); the backward pass lifts small incoming gradients by a power of two, so the numbers hold at any loss scale; "
                             "x2_plan=0 = pairs everywhere (5.8e-6)",
                  "value": round(pv, 3), "unit": "images/sec", "steps": parity_res["steps"], "warmup": parity_res["warmup"],
                  "ms_per_step": round(parity_res["dt"] / parity_res["steps"] * 1e3, 2),
                  "generator_tflops_per_gpu": round(pv / world * flop_per_image / 1e12, 2), "loss": parity_res["loss"],
                  "weight_gradients": "stream chunks of conv5 / tail: three tap-products (X_hi G_hi + 2^-12 (X_hi G_lo + X_lo G_hi)); conv1..conv4: G is read as a single f16 tensor; growth-plane X chunks: their hi tensor"}
            if parity_hi is not None:
                pm["hi_only_weight_gradients"] = {"knob": "RESR_X2_WGRAD_PRODUCTS=1 (opt-in)", "value": round(rate(parity_hi), 3), "unit": "images/sec",
                                                  "ms_per_step": round(parity_hi["dt"] / parity_hi["steps"] * 1e3, 2),
                                                  "gradient_error": "worst tensor 2.8-5.0e-4 against the all-pairs plan under a dense random cotangent, 2.4-3.1e-4 under the L1 loss (conv4: the L1 gradient has ONE magnitude, whose f16 rounding is systematic) -- profiles/r05_x2_plan_validate_hi_only.json; inside 1e-3, not inside the 5e-4 ship rule"}
            if parity_p7 is not None:
                pm["without_mx_stages"] = {"knob": "x2_plan=59 / RESR_X2_PLAN=59 (round 5's default: backward-data reads the growth-plane gradients as single f16, 50 f16 stages per block)",
                                           "value": round(rate(parity_p7), 3), "unit": "images/sec", "ms_per_step": round(parity_p7["dt"] / parity_p7["steps"] * 1e3, 2)}
            if "roofline" in parity_res:
                r = parity_res["roofline"]
                pm["roofline"] = {k: r[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "avg_launch_ms", "per_instance", "vs_sustained") if k in r}
                pm["roofline"]["note"] = "achieved = algorithmic FLOP (2*9*cin*cout*px) per second; the matrix pipe executes 3x that"
            try:
                x, ys = parity_probe(main_res["state_dict"])
                pm["probe"] = {"input": "1x3x24x24, seeded; weights of the timed model after its steps",
                               "max_abs_vs_strict_f32_mfma": {k: float((v - ys["strict"]).abs().max()) for k, v in ys.items() if k != "strict"}}
                if world == 1 and not args.no_cpu_baseline:
                    import tempfile
                    probe_path = os.path.join(tempfile.mkdtemp(prefix="resr_probe_"), "probe.pt")
                    torch.save({"x": x, "sd": {k: v.cpu() for k, v in main_res["state_dict"].items()}, "y": ys}, probe_path)
            except Exception as e:  # pragma: no cover
                probe_err = repr(e)
                pm["probe"] = {"error": probe_err}
            if world == 1:
                try:
                    pm["gradient_probe"] = gradient_probe(main_res["state_dict"], B, lr_edge)
                except Exception as e:  # pragma: no cover
                    pm["gradient_probe"] = {"error": repr(e)}
            out["parity_mode"] = pm
        # a fixed, kernel-independent figure of THIS box (the power-cap frontier measured before the timed steps): lets a reader tell
        # box-to-box spread (+-5 % for one build) from a regression when the records of two rounds are compared
        fr = _LIVE_FRONTIER       # only the live measurement: the committed fallback of sustained_frontier() is another box
        if fr:
            out["box_reference"] = {"matrix_alone_tflops": round(fr[0] * 1e3, 1), "stream_tbs": fr[1], "matrix_next_to_stream_tflops": round(fr[2] * 1e3, 1),
                                    "source": fr[3], "how": "resr_debug_sustained: 256 workgroups of MFMA waves (alone / next to an LDS-DMA stream), 1.5 s per arm"}
        if world == 1 and not args.no_other_configs:
            out["other_configs"] = other_configs(args)
            if fr:
                out["other_configs"]["box_reference"] = out["box_reference"]
        if args.isolated_probe:
            rows = probe_conv_kernels(B, lr_edge, args.precision)
            out["conv_probe_isolated"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items() if k != "flop"}
                                          for r in rows]
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"], oracle_probe = cpu_baseline(probe_path)
                if oracle_probe and "parity_mode" in out and "probe" in out["parity_mode"]:
                    out["parity_mode"]["probe"]["max_abs_vs_cpu_oracle_fp32"] = oracle_probe
            except Exception as e:  # pragma: no cover
                out["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
