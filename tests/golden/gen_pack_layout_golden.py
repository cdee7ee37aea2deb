"""Writes tests/golden/pack_layout.json: the chunk count, the SHA-256 of the table's bytes and every size the library reports, for the
descriptors tests/test_pack_layout.py walks (`collect` below is shared with the test), plus the VGG19 table of ContentLoss.

    python tests/golden/gen_pack_layout_golden.py

All of it is host arithmetic: no GPU.  The fixture was written once, by the commit BEFORE csrc/packed_layout.h existed, and is the
statement that the packed layout did not move; regenerate it only for a deliberate layout change.  `vgg_table` is that commit's own
Python loop of ContentLoss._pack, kept here as the independent spelling of the VGG table.
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "pack_layout.json")
FAKE_WORKSPACE = 1 << 20   # the discriminator's table points into its workspace: pointer arithmetic on this address only

VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512]


def sha(chunks):
    return hashlib.sha256(bytes(chunks)).hexdigest()


def table(L, call, what):
    host = L.fetch_pack_table(call, what)
    return {"chunks": len(host), "sha256": sha(host)}


def collect(L):
    """name -> everything the library reports for that descriptor."""
    lib = L.lib()
    out = {}
    dtypes = (("f16", L.RESR_F16), ("f32", L.RESR_F32), ("f16x2", L.RESR_F16X2))
    for upscale in (1, 2, 4):
        for dname, dtype in dtypes:
            for plan in ((0, 763, 2401) if dtype == L.RESR_F16X2 else (0,)):
                rec = {}
                for training in (0, 1):
                    d = L.GeneratorDesc(1, 24, 24, 3, 3, upscale, 2, dtype, training, 0, plan, 0)
                    r = C.byref(d)
                    rec[f"training{training}"] = {
                        "table0": table(L, lambda c, n: lib.resr_generator_pack_table(r, 0, c, n), "generator table"),
                        "table1": table(L, lambda c, n: lib.resr_generator_pack_table(r, 1, c, n), "generator table"),
                        "packed_bytes0": lib.resr_generator_packed_bytes(r, 0),
                        "packed_bytes1": lib.resr_generator_packed_bytes(r, 1),
                        "mx_offset": lib.resr_generator_mx_offset(r),
                        "workspace_bytes": lib.resr_generator_workspace_bytes(r),
                        "chain_state_bytes": lib.resr_generator_chain_state_bytes(r),
                        "param_count": lib.resr_generator_param_count(r),
                    }
                out[f"generator/x{upscale}/{dname}/plan{plan}"] = rec
    for upscale in (1, 2, 3, 4):
        for aname, act in (("prelu", L.COMPACT_PRELU), ("lrelu", L.COMPACT_LRELU)):
            for dname, dtype in dtypes:
                d = L.CompactDesc(1, 5, 7, 2, upscale, act, dtype, 0)
                r = C.byref(d)
                out[f"compact/x{upscale}/{aname}/{dname}"] = {
                    "table": table(L, lambda c, n: lib.resr_compact_pack_table(r, c, n), "compact table"),
                    "packed_bytes": lib.resr_compact_packed_bytes(r),
                    "workspace_bytes": lib.resr_compact_workspace_bytes(r),
                    "param_count": lib.resr_compact_param_count(r),
                }
    for dname, dtype in dtypes:
        for training in (0, 1):
            d = L.DiscriminatorDesc(1, 16, 16, dtype, training, training)
            r = C.byref(d)
            out[f"discriminator/{dname}/training{training}"] = {
                "table": table(L, lambda c, n: lib.resr_discriminator_pack_table(r, C.c_void_p(FAKE_WORKSPACE), c, n), "discriminator table"),
                "workspace_bytes": lib.resr_discriminator_workspace_bytes(r),
                "param_count": lib.resr_discriminator_param_count(),
                "uv_count": lib.resr_discriminator_uv_count(),
            }
    return out


def vgg_table(L):
    """The VGG19 table as ContentLoss._pack typed it before the library emitted it: (host chunks, forward groups, backward groups,
    total elements); groups: conv index -> [(element offset, mt), ...]."""
    def r32(v):
        return (v + 31) // 32 * 32
    chunks, fwd, bwd, off, src = [], {}, {}, 0, 0
    idx, cin = 0, 3
    for v in VGG_CFG:
        if v == "M":
            idx += 1
            continue
        cout = v
        for tab, m_real, k_real, tr in ((fwd, cout, cin, 0), (bwd, cin, cout, 1)):
            gl = []
            for g0 in range(0, r32(m_real), 64):
                mt = min(64, r32(m_real) - g0) // 32
                gl.append((off, mt))
                for ck in range(r32(k_real) // 32):
                    chunks.append(L.PackChunk(src, off, cout, cin, g0, max(0, min(64, m_real - g0)), ck * 32,
                                              max(0, min(32, k_real - ck * 32)), mt, tr, 1.0, 0, None))
                    off += 9 * mt * 1024
            tab[idx] = gl
        src += cout * cin * 9
        idx += 2
        cin = v
    return (L.PackChunk * len(chunks))(*chunks), fwd, bwd, off


def vgg_record(host, fwd, bwd, elems):
    def groups(t):
        return {str(k): [list(g) for g in v] for k, v in sorted(t.items())}
    return {"chunks": len(host), "sha256": sha(host), "elems": elems, "fwd": groups(fwd), "bwd": groups(bwd)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
    import real_esrgan_pytorch_amd as R
    golden = collect(R._lib)
    golden["vgg19"] = vgg_record(*vgg_table(R._lib))
    with open(OUT, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, len(golden), "records")
