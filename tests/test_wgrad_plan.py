"""The host planner of the batched weight-gradient launches (csrc/wgrad.hip, wgrad_batch) through resr_debug_wgrad_batch_plan: every
table of every batch the networks issue equals tests/golden/wgrad_plans.json (written by tests/golden/gen_wgrad_plan_golden.py BEFORE
the planner's walk over a batch got its one definition), integer for integer, refusals with their text.  The fixture is a recording,
so each accepted case is also checked from first principles: where the slabs lie, which job every quad slot computes, what the
reduction reads.  All host arithmetic: no GPU."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_wgrad_plan_golden", os.path.join(HERE, "golden", "gen_wgrad_plan_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(HERE, "golden", "wgrad_plans.json")) as f:
    GOLDEN = json.load(f)
K_SLAB = 9 * 1024 + 32   # floats per (job, split): csrc/wgrad.h


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    return R._lib


def test_fixture_covers_the_generator_cases():
    assert list(GOLDEN) == list(gen.cases())
    for name, case in gen.cases().items():
        assert GOLDEN[name]["case"] == case, name


def uncapped_mx_factor(n_mx, splits):
    """The factor the MX launch's pixel splits take over `splits` before the cap of two tiles per workgroup: three quads x k x splits
    of about one residency round of 256 workgroups, k = 1..4 (what wgrad_batch_partial_bytes sizes for)."""
    if n_mx <= 0:
        return 1
    return max(1, min(4, 256 // ((n_mx + 3) // 4 * ((splits + 7) // 8 * 8))))


def check_principles(case, res):
    t = dict(zip(("jobs", "products", "mx_jobs", "quads", "quads_mx", "splits_mx", "splits_c", "fast_addr", "batch_jobs", "batch_quads",
                  "partial_floats"), res["totals"]))
    jobs, reduce, splits = res["jobs"], res["reduce"], case["splits"]
    assert len(jobs) == t["jobs"] == t["batch_jobs"] and len(reduce) == t["products"]
    assert t["mx_jobs"] == sum(j[6] for j in jobs)
    assert t["splits_mx"] % splits == 0 and t["splits_c"] == (t["splits_mx"] if t["mx_jobs"] else 0)
    tiles = (case["w"] + 31) // 32 * ((case["h"] + 7) // 8) * case["n"]
    assert t["splits_mx"] == splits or t["splits_mx"] <= tiles // 2
    # slab regions: disjoint, contiguous in job order, splits (MX jobs: splits_mx) slabs each
    end = 0
    for j in jobs:
        assert j[3] == end
        assert j[6] == (1 if j[2] == 3 else 0)
        end += (t["splits_mx"] if j[6] else splits) * K_SLAB
    # ... up to the size the planners ask for -- which assumes the uncapped MX factor (it is asked before the geometry is known)
    k = uncapped_mx_factor(t["mx_jobs"], splits)
    assert t["splits_mx"] <= k * splits
    assert end == t["partial_floats"] - t["mx_jobs"] * (k * splits - t["splits_mx"]) * K_SLAB
    # the reduction: product by product the jobs' slabs, part 0 first; the bias where chunk 0 of a convolution with a bias is summed
    ji = 0
    for p in reduce:
        slab_off, slab_b, slab_c, co_base, ci_base, cout, cin_real, want_bias, c_bias, conv, db = p
        cv = case["convs"][conv]
        assert (cout, cin_real, db) == (cv[3], cv[2], cv[5]) and co_base % 32 == 0 and co_base < cv[4] and ci_base % 32 == 0 and ci_base < cv[0]
        assert want_bias == (1 if ci_base == 0 and cv[5] else 0)
        mine = []
        while ji < len(jobs) and (not mine or jobs[ji][2] != 0):
            mine.append(jobs[ji])
            ji += 1
        parts = [j[2] for j in mine]
        assert parts[0] == 0 and parts == sorted(set(parts)) and not (3 in parts and len(parts) > 2)
        assert slab_off == mine[0][3]
        assert slab_b == next((j[3] for j in mine if j[2] == 1), -1)
        assert slab_c == next((j[3] for j in mine if j[2] in (2, 3)), -1)
        assert c_bias == (1 if 3 in parts and want_bias else 0)
        for j in mine:
            assert j[4] == (want_bias if j[2] != 2 else 0)
            # (x_hi, g_lo) reads part 0's X, (x_lo, g_hi) its G, an MX job the q tensors of both; strides and tap pattern are the chunk's
            assert (j[0] == mine[0][0]) == (j[2] < 2) and (j[1] == mine[0][1]) == (j[2] in (0, 2))
            assert j[5] == mine[0][5] and j[7:] == mine[0][7:]
    assert ji == len(jobs)
    if t["quads"]:
        assert t["batch_quads"] == t["quads"]
    # quads: every job in exactly one slot of a quad of its kind, on that slot's operands
    for kind, quads in ((0, res["quads"]), (1, res["quads_mx"])):
        assert len(quads) == (t["quads_mx"] if kind else t["quads"])
        want = {j[3]: j for j in jobs if j[6] == kind}
        if not quads:
            assert kind == 1 and not want or kind == 0 and (case["dtype"] == "RESR_F32" or not t["fast_addr"])
            continue
        seen = []
        for q in quads:
            for s in range(4):
                if q[s] < 0:
                    assert not (q[4] >> s) & 0x111
                    continue
                j = want[q[s]]
                seen.append(q[s])
                assert (q[6 + (s & 1)], q[8 + (s >> 1)]) == (j[0], j[1])
                assert (q[4] >> s) & 1 == j[4] and (q[4] >> (8 + s)) & 1 == kind and not (q[4] >> (4 + s)) & 1
                assert (q[5] >> (8 * (s & 1))) & 0xff == j[5]
        assert sorted(seen) == sorted(want)


@pytest.mark.parametrize("name", list(GOLDEN))
def test_plan_equals_the_recorded_one(L, name):
    case, want = GOLDEN[name]["case"], GOLDEN[name]["result"]
    got = gen.run(L, case)
    assert got == want
    if got["status"] == 0:
        check_principles(case, got)
    else:
        assert got["status"] == L.RESR_ERR_ARG and got["error"]


def test_job_counts_of_the_exact16_families(L):
    """The counts csrc/generator.hip (carve) sizes the slab buffer by."""
    counts = {name: GOLDEN[f"x2/{name}@16x64x64"]["result"]["totals"][:3] for name in
              ("dense_block/all_pairs", "dense_block/gg_single", "dense_block/gg_single+wx_pairs", "dense_block/gg_single+wx_pairs+g_hi",
               "dense_block/mx_wgrad", "tail_64_64", "tail_64_64/mx")}
    assert counts == {"dense_block/all_pairs": [78, 26, 0], "dense_block/gg_single": [68, 26, 0], "dense_block/gg_single+wx_pairs": [54, 26, 0],
                      "dense_block/gg_single+wx_pairs+g_hi": [46, 26, 0], "dense_block/mx_wgrad": [38, 26, 12], "tail_64_64": [12, 4, 0],
                      "tail_64_64/mx": [8, 4, 4]}
    assert GOLDEN["f16/rrdb@16x64x64"]["result"]["totals"][:2] == [78, 78]


def test_one_slab_count_per_launch_is_enforced(L):
    """ReduceArgs.splits_c is one value per launch: a batch in which one product's slab_c region was written by an f16 (x_lo, g_hi) job
    (`splits` slabs) while the MX jobs run on their own, larger split count is refused before any launch; where the two counts agree
    the same batch is planned (recorded at 1 x 24 x 24)."""
    case = dict(gen.cases()["x2/mx_beside_f16@1x24x24"])
    assert gen.run(L, case)["status"] == 0
    n, h, w, splits = gen.GEOMETRIES["16x64x64"]
    case.update(n=n, h=h, w=w, splits=splits)
    got = gen.run(L, case)
    assert got["status"] == L.RESR_ERR_ARG
    assert "splits" in got["error"] and "MX" in got["error"]
    # either convolution alone is planned at that geometry
    for c in case["convs"]:
        assert gen.run(L, dict(case, convs=[c]))["status"] == 0
