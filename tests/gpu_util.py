"""Test plumbing for the -m gpu parity tests: layout conversion and single-conv packing.

The product is only reached through the C-ABI (real_esrgan_pytorch_amd._lib); torch is used here
for device memory and for converting between the oracle's NCHW fp32 and the library's layouts.
"""
import ctypes as C

import numpy as np
import torch

import real_esrgan_pytorch_amd as R
from tests import disc_helpers_ref as ref

L = R._lib


def tdtype(dtype):
    return torch.float16 if dtype == L.RESR_F16 else torch.float32


def to_nhwc(x_nchw, dtype, c_pad=None, stride=None, offset=0):
    """NCHW fp32 (cpu) -> device NHWC tensor [N,H,W,stride] holding the channels at `offset`."""
    n, c, h, w = x_nchw.shape
    c_pad = c_pad or c
    stride = stride or c_pad
    buf = torch.zeros(n, h, w, stride, dtype=tdtype(dtype), device="cuda")
    buf[..., offset:offset + c] = x_nchw.permute(0, 2, 3, 1).to(tdtype(dtype)).cuda()
    return buf


def from_nhwc(buf, c, offset=0):
    return buf[..., offset:offset + c].float().cpu().permute(0, 3, 1, 2).contiguous()


def pack_conv(weight, dtype, transposed=False, scale=1.0):
    """Pack one OIHW fp32 conv weight through resr_pack_weights (forward or backward-data form)."""
    cout, cin = weight.shape[:2]
    m_real, k_real = (cin, cout) if transposed else (cout, cin)
    m_pad = (m_real + 31) // 32 * 32
    k_pad = (k_real + 31) // 32 * 32
    mt = m_pad // 32
    nck = k_pad // 32
    chunks = (L.PackChunk * nck)()
    for ck in range(nck):
        kc = min(32, k_real - ck * 32)
        chunks[ck] = L.PackChunk(0, ck * 9 * mt * 1024, cout, cin, 0, m_real, ck * 32, kc, mt,
                                 1 if transposed else 0, scale, 0, None)
    table = torch.frombuffer(bytearray(bytes(chunks)), dtype=torch.uint8).cuda()
    arena = weight.reshape(-1).float().cuda()
    es = {L.RESR_F16: 2, L.RESR_F32: 4, L.RESR_F16X2: 6}[dtype]   # exact16: three f16 blocks per chunk
    packed = torch.zeros(nck * 9 * mt * 1024 * es + 16384, dtype=torch.uint8, device="cuda")
    L.check(L.lib().resr_pack_weights(L.ptr(table), nck, L.ptr(arena), L.ptr(packed), dtype, L.stream_ptr()),
            "resr_pack_weights")
    return packed


def quant(x, dtype):
    """Round a cpu fp32 tensor to the storage type the kernel will see."""
    return x.to(tdtype(dtype)).float()


def sptr(t, elem_offset=0):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + elem_offset * t.element_size())


# ---- guarded outputs and operands of the kernel-level tests (test_gpu_disc_helpers.py, test_gpu_layout_kernels.py) ---------------
GUARD = 64
SENT = {np.dtype(np.float16): 0x7E5A, np.dtype(np.float32): 0x7FC5A5A5, np.dtype(np.uint8): 0xA5}   # NaN payloads no kernel produces
INT = {np.dtype(np.float16): np.int16, np.dtype(np.float32): np.int32, np.dtype(np.uint8): np.uint8}
TORCH = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}
TINT = {np.dtype(np.float16): torch.int16, np.dtype(np.float32): torch.int32, np.dtype(np.uint8): torch.uint8}

def np_type(L, dtype):
    return np.dtype(np.float32 if dtype == L.RESR_F32 else np.float16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """`count` elements of `np_dtype` between two guards, everything pre-filled with the sentinel."""

    def __init__(self, count, np_dtype):
        self.dt, self.count = np.dtype(np_dtype), int(count)
        self.t = torch.empty(self.count + 2 * GUARD, dtype=TORCH[self.dt], device="cuda")
        self.t.view(TINT[self.dt]).fill_(self._sent())
        self.ptr = self.t.data_ptr() + GUARD * self.dt.itemsize

    def _sent(self):
        s = SENT[self.dt]
        return int(np.array(s, dtype=np.uint32).astype(INT[self.dt])) if self.dt != np.uint8 else s

    def load(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype == self.dt and a.size == self.count
        self.t[GUARD:GUARD + self.count] = dev(a)
        return self

    def read(self, written=True):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        i = a.view(INT[self.dt])
        assert (i[:GUARD] == self._sent()).all(), "the guard in front of the output was written"
        assert (i[GUARD + self.count:] == self._sent()).all(), "the guard behind the output was written"
        body = a[GUARD:GUARD + self.count].copy()
        if written:
            missed = np.flatnonzero(body.view(INT[self.dt]) == self._sent())
            assert missed.size == 0, f"{missed.size} elements in range never written, first at {missed[0]}"
        return body


class Operand:
    """An input tensor as the kernel sees it.  exact: the float64 value of every element; v32: what the kernel loads (fp32; for a
    pair the single rounding of exact); flat: the stored elements (pair: hi tensor, then lo tensor directly behind)."""

    def __init__(self, L, dtype, base=None, hi=None, lo=None):
        if dtype == L.RESR_F16X2:
            if hi is None:
                hi, lo = ref.pair_split(np.asarray(base, dtype=np.float32).astype(np.float64))
            self.hi, self.lo = np.asarray(hi, dtype=np.float16), np.asarray(lo, dtype=np.float16)
            self.exact = ref.pair_join(self.hi, self.lo)
            self.flat = np.concatenate([self.hi.reshape(-1), self.lo.reshape(-1)])
        else:
            q = np.asarray(base, dtype=np.float32).astype(np_type(L, dtype))
            self.hi, self.lo = q, None
            self.exact = q.astype(np.float64)
            self.flat = q.reshape(-1)
        self.v32 = self.exact.astype(np.float32)
        self.shape = self.exact.shape
        self.t = dev(self.flat)
        self.ptr = self.t.data_ptr()


# ---- the record of the conv / weight-gradient judgements (test_gpu_kernels.py, test_gpu_x2_plan.py) -------------------------------
def merge_conv_diag(diag_dir, records, restart=False):
    """Add `records` ({case: record of tests/conv_ref.judge + dtype, kind}) to <diag_dir>/test_gpu_conv_kernels.json and renew its
    "worst" table (the worst ratio per dtype).  restart: drop what an earlier run left first."""
    import json
    import os
    path = os.path.join(diag_dir, "test_gpu_conv_kernels.json")
    if restart and os.path.exists(path):
        os.remove(path)
    cases = {}
    if os.path.exists(path):
        with open(path) as f:
            cases = json.load(f)["cases"]
    cases.update(records)
    worst = {}
    for name, rec in cases.items():
        if rec["dtype"] not in worst or rec["ratio"] > worst[rec["dtype"]]["ratio"]:
            worst[rec["dtype"]] = {"case": name, "ratio": rec["ratio"]}
    with open(path, "w") as f:
        json.dump({"worst": worst, "cases": cases}, f, indent=1, sort_keys=True)
