"""Writes tests/golden/wgrad_plans.json: every table the host planner of csrc/wgrad.hip (wgrad_batch) builds for the batched
weight-gradient launches the three networks issue, as resr_debug_wgrad_batch_plan (include/resr_debug.h) reports them.

    python tests/golden/gen_wgrad_plan_golden.py

All of it is host arithmetic: no GPU.  `cases` and `run` are shared with tests/test_wgrad_plan.py, which replays every record.  The
fixture was written once, by the planner as it stood BEFORE its walk over a batch's tap-products got its one definition (the debug
entry on top of it, wgrad_batch's table-building block moved into a function of its own and nothing else), and is the statement that
no table moved since; regenerate it only for a deliberate change of the plan.  The batches are described the way csrc/generator.hip
(generator_backward), csrc/disc_native.hip (wgrad_layer) and csrc/compact.hip (compact_backward) describe theirs.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "wgrad_plans.json")

UPSAMPLE_IN = "up"
# (n, h, w, splits): 3 tiles -- the MX launch's factor is capped at tiles / 2; 256 tiles -- the MX launch takes k > 1 times the splits;
# more than 2^24 pixels -- fast_addr = 0: the pair kernel, and no MX job
GEOMETRIES = {"1x24x24": (1, 24, 24, 1), "16x64x64": (16, 64, 64, 32), "1x4096x4104": (1, 4096, 4104, 8)}


def conv(cin, cout, *, cout_pad=None, cin0=None, cin_real=None, bias=1, xp=0, gp=0, xs=None, x1s=0, gs=None, xb=0, x1b=0, gb=0, gt=0,
         g_lo=1, g_lo_bias_only=0, x_pair_chunks=0, x_single_g_hi=0, q=0, s2d=0, unscale=1):
    """One convolution as the RESR_DEBUG_WGRAD_CONV_FIELDS integers of resr_debug_wgrad_batch_plan, in the header's order."""
    cout_pad = cout_pad if cout_pad is not None else (cout + 31) // 32 * 32
    cin0 = cin if cin0 is None else cin0
    xs = xs if xs is not None else (32 if xp else cin0)
    gs = gs if gs is not None else (32 if gp else cout_pad)
    return [cin, cin0, cin if cin_real is None else cin_real, cout, cout_pad, bias, xp, gp, xs, x1s, gs, xb, x1b, gb, gt,
            g_lo, g_lo_bias_only, x_pair_chunks, x_single_g_hi, q, s2d, unscale]


def dense_block(b=0, *, gg_single=0, gg_store_single=0, wx_pairs=0, x_single_g_hi=0, mx_wgrad=0):
    """conv1..conv5 of dense block `b` as generator_backward hands them over: X = the first 64 + 32 (k - 1) channels of the block's
    chunk-planar workspace; G = plane 4 - k of the block's gradient slab (conv1..conv4), the incoming gradient's two planes (conv5)."""
    cs = [conv(64 + 32 * (k - 1), 32, xp=1, gp=1, xb=b, gb=2 * b, gt=4 - k, g_lo=0 if gg_store_single else 1,
               g_lo_bias_only=1 if gg_single and not gg_store_single else 0, x_pair_chunks=wx_pairs, q=mx_wgrad) for k in range(1, 5)]
    cs.append(conv(192, 64, xp=1, gp=1, xb=b, gb=2 * b + 1, x_pair_chunks=wx_pairs, x_single_g_hi=x_single_g_hi, q=mx_wgrad))
    return cs


def rrdb(**kw):
    return [c for b in range(3) for c in dense_block(b, **kw)]


def disc_down1(parts):
    """DOWN1 of the discriminator (64 -> 128, 4x4 / stride 2, no bias): X = the space-to-depth image of 4 x 64 channels; as many
    64-channel convolutions per launch as 96 tap-products and 80 products allow -- both, whether `parts` is 1 or 3."""
    assert min(96 // (8 * parts), 80 // 8) * 32 >= 128
    return [conv(256, 64, bias=0, xs=256, gs=128, gt=2 * i, s2d=64) for i in range(2)]


F16, F32, X2 = "RESR_F16", "RESR_F32", "RESR_F16X2"
TAIL = dict(xp=1, gp=1)   # the generator's convolutions outside the trunk: chunk-planar X and G


def batches():
    """name -> (dtype, convs, flags, environment)."""
    out = {}
    for dname, dt in (("f16", F16), ("f32", F32)):
        out[f"{dname}/dense_block"] = (dt, dense_block(), 0, {})
        out[f"{dname}/conv_64_64"] = (dt, [conv(64, 64, **TAIL)], 0, {})
    out["f16/rrdb"] = (F16, rrdb(), 0, {})
    out["f16/conv1_32_64"] = (F16, [conv(32, 64, cin_real=3, gp=1)], 0, {})
    out["f16/conv4_64_32"] = (F16, [conv(64, 3, xp=1)], 0, {})
    out["f16/compact_64_64"] = (F16, [conv(64, 64)], 0, {})
    out["f16/compact_first"] = (F16, [conv(32, 64, cin_real=3)], 0, {})
    out["f16/compact_last"] = (F16, [conv(64, 48)], 0, {})
    out["f16/two_segment"] = (F16, [conv(96, 64, cin0=64, x1s=32, x1b=1, unscale=0)], 0, {})
    out["f16/upsample_in"] = (F16, [conv(64, 64, **TAIL)], UPSAMPLE_IN, {})
    out["f16/disc_down1_s2d"] = (F16, disc_down1(1), 0, {})
    out["f32/disc_down1_s2d"] = (F32, disc_down1(1), 0, {})
    out["x2/disc_down1_s2d"] = (X2, disc_down1(3), 0, {})
    gg = dict(gg_single=1)
    gw = dict(gg_single=1, wx_pairs=2)
    gh = dict(gg_single=1, wx_pairs=2, x_single_g_hi=1)
    out["x2/dense_block/all_pairs"] = (X2, dense_block(), 0, {})
    out["x2/dense_block/gg_single"] = (X2, dense_block(**gg), 0, {})
    out["x2/dense_block/gg_single+wx_pairs"] = (X2, dense_block(**gw), 0, {})
    out["x2/dense_block/gg_single+wx_pairs+g_hi"] = (X2, dense_block(**gh), 0, {})
    out["x2/dense_block/gg_store_single"] = (X2, dense_block(gg_single=1, gg_store_single=1), 0, {})
    out["x2/dense_block/gg_store_single+wx_pairs+g_hi"] = (X2, dense_block(gg_store_single=1, **gh), 0, {})
    out["x2/dense_block/mx_wgrad"] = (X2, dense_block(mx_wgrad=1, **gh), 0, {})
    out["x2/dense_block/mx_wgrad_alone"] = (X2, dense_block(mx_wgrad=1, wx_pairs=2), 0, {})
    out["x2/tail_64_64"] = (X2, [conv(64, 64, **TAIL)], 0, {})
    out["x2/tail_64_64/mx"] = (X2, [conv(64, 64, q=1, **TAIL)], 0, {})
    out["x2/tail_64_32/mx"] = (X2, [conv(64, 3, xp=1, q=1)], 0, {})
    out["x2/tail_upsample_in/mx"] = (X2, [conv(64, 64, q=1, **TAIL)], UPSAMPLE_IN, {})
    out["x2/two_segment"] = (X2, [conv(96, 32, cin0=64, x1s=32, x1b=1, unscale=0)], 0, {})
    one = {"RESR_X2_WGRAD_PRODUCTS": "1"}
    out["x2/products1/dense_block/mx_wgrad"] = (X2, dense_block(mx_wgrad=1, **gh), 0, one)
    out["x2/products1/rrdb"] = (X2, rrdb(**gh), 0, one)
    # one convolution with q tensors beside one without: its (x_lo, g_hi) jobs and the MX jobs share ReduceArgs.splits_c
    out["x2/mx_beside_f16"] = (X2, [conv(64, 64, q=1, **TAIL), conv(64, 64, xb=1, gb=1, **TAIL)], 0, {})
    # what the planner refuses
    out["refused/jobs"] = (X2, dense_block(0) + dense_block(1), 0, {})
    out["refused/products"] = (F16, rrdb() + [conv(64, 64, xb=3, gb=6, **TAIL)], 0, {})
    out["refused/unscale"] = (F16, [conv(64, 64, **TAIL), conv(64, 64, xb=1, gb=1, unscale=2, **TAIL)], 0, {})
    out["refused/cout_pad_96"] = (F16, [conv(64, 64, **TAIL), conv(64, 96, xb=1, gb=1, **TAIL)], 0, {})
    return out


# the geometries a batch is recorded at (default: all three)
ONLY = {"x2/mx_beside_f16": ("1x24x24",),   # (at 16x64x64 splits_mx != splits: tests/test_wgrad_plan.py asserts the refusal)
        "refused/jobs": ("16x64x64",), "refused/products": ("16x64x64",), "refused/unscale": ("16x64x64",),
        "refused/cout_pad_96": ("16x64x64",)}


def cases():
    """name -> {"dtype", "convs", "flags", "env", "n", "h", "w", "splits"}, in the fixture's order."""
    out = {}
    for name, (dt, convs, flags, env) in batches().items():
        for gname in ONLY.get(name, GEOMETRIES):
            n, h, w, splits = GEOMETRIES[gname]
            out[f"{name}@{gname}"] = {"dtype": dt, "convs": convs, "flags": flags, "env": env, "n": n, "h": h, "w": w, "splits": splits}
    out["refused/odd_h_upsample_in@1x25x24"] = {"dtype": F16, "convs": [conv(64, 64, **TAIL)], "flags": UPSAMPLE_IN, "env": {},
                                               "n": 1, "h": 25, "w": 24, "splits": 1}
    return out


def run(L, case):
    """The library's answer for one case: {"status": 0, "totals", "jobs", "reduce", "quads", "quads_mx"} with one row of integers per
    job / product / quad, or {"status": < 0, "error": text}."""
    lib = L.lib()
    nf = (L.RESR_DEBUG_WGRAD_CONV_FIELDS, L.RESR_DEBUG_WGRAD_TOTALS, L.RESR_DEBUG_WGRAD_JOB_FIELDS, L.RESR_DEBUG_WGRAD_REDUCE_FIELDS,
          L.RESR_DEBUG_WGRAD_QUAD_FIELDS)
    flat = [v for c in case["convs"] for v in c]
    assert all(len(c) == nf[0] for c in case["convs"])
    totals, jobs, reduce = (C.c_int32 * nf[1])(), (C.c_int32 * (96 * nf[2]))(), (C.c_int32 * (80 * nf[3]))()
    quads, quads_mx = (C.c_int32 * (40 * nf[4]))(), (C.c_int32 * (40 * nf[4]))()
    saved = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        rc = lib.resr_debug_wgrad_batch_plan((C.c_int32 * len(flat))(*flat), len(case["convs"]), getattr(L, case["dtype"]), case["n"],
                                             case["h"], case["w"], L.CONV_UPSAMPLE_IN if case["flags"] == UPSAMPLE_IN else 0,
                                             case["splits"], totals, jobs, reduce, quads, quads_mx)
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    if rc != 0:
        return {"status": rc, "error": lib.resr_last_error().decode()}

    def rows(buf, count, width):
        return [list(buf[i * width:(i + 1) * width]) for i in range(count)]
    t = list(totals)
    return {"status": 0, "totals": t, "jobs": rows(jobs, t[0], nf[2]), "reduce": rows(reduce, t[1], nf[3]), "quads": rows(quads, t[3], nf[4]),
            "quads_mx": rows(quads_mx, t[4], nf[4])}


def dumps(golden):
    """One case per line: the fixture stays small and a changed table shows as one changed line."""
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'), sort_keys=True)}" for k, v in golden.items()) + "\n}\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    golden = {name: {"case": case, "result": run(R._lib, case)} for name, case in cases().items()}
    with open(OUT, "w") as f:
        f.write(dumps(golden))
    print(OUT, len(golden), "records", os.path.getsize(OUT), "bytes")
