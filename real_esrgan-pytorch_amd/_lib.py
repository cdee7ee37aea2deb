"""ctypes binding of csrc/libresr_hip.so (C-ABI declared in include/resr.h and include/resr_debug.h).

The headers are the single declaration: at import _header.py reads both and every prototype, structure and constant here is what they
say; nothing of the ABI is typed in a second time, and a declaration the reader does not understand fails the import.
The product path has no CPU or PyTorch fallback: if the shared library is missing, `lib()` raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# RESR_LIB_PATH: experiment knob -- load a variant build (tools/build_variant.py) for same-box A/B timing
LIB_PATH = os.environ.get("RESR_LIB_PATH") or os.path.join(_HERE, "csrc", "libresr_hip.so")

_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")   # where csrc/build.py finds the headers too
_ABI = _header.read(os.path.join(_INCLUDE, "resr.h"), os.path.join(_INCLUDE, "resr_debug.h"))

# The structures under their header names without "Resr", fields in header order: ConvDesc, WgradDesc, PackChunk, GeneratorDesc, CompactDesc,
# YuvDesc, ImageDesc, DiscriminatorDesc, NiqeDesc, NiqeScoreDesc, FullRefDesc, FullRefPlanesDesc, ProfEntry.  The constants: a member of one of these families loses its RESR_ prefix (RESR_CONV_LRELU -> CONV_LRELU);
# everything else keeps the header's name (RESR_F16, RESR_F32, RESR_F16X2, RESR_OK, RESR_ERR_*, RESR_VERSION).
_FAMILIES = ("CONV_", "X2_PLAN_", "COMPACT_", "YUV_")
globals().update({cls.__name__: cls for cls in _ABI.structs.values()})
globals().update({(name[5:] if name[5:].startswith(_FAMILIES) else name): value for name, value in _ABI.consts.items()})
_PROTOS = _ABI.protos   # name -> (restype, [argtypes]) of every function the two headers declare

# the named "output parity" training plan: bits 0 + 5 + 6 (the inference MX forward) + 8 (f16 backward) + 11 (MX_TRAIN_FORWARD)
X2_PLAN_OUTPUT_PARITY = (X2_PLAN_GROWTH_F16_INFER | X2_PLAN_GROWTH_W16_INFER | X2_PLAN_MX_INFER | X2_PLAN_F16_BACKWARD
                         | X2_PLAN_MX_TRAIN_FORWARD)   # 2401


def x2_plan_error(plan: int):
    """None for a plan the library accepts (with RESR_F16X2), else the library's text for the first rule the plan breaks: the prerequisite
    table of include/resr.h, which csrc/generator.hip (resolve_x2_plan) alone checks."""
    d = GeneratorDesc(1, 24, 24, 3, 3, 4, 2, RESR_F16X2, 0, 0, plan, 0)   # valid in everything but, perhaps, x2_plan
    return None if lib().resr_generator_param_count(C.byref(d)) else lib().resr_last_error().decode()


# What the module itself has to know about a valid exact16 plan (everything else is the library's business):
def x2_plan_f16_backward(plan: int) -> bool:
    """The backward pass takes a RESR_F16 packing of the weight table."""
    return bool(plan & X2_PLAN_F16_BACKWARD)


def x2_plan_packs_mx(plan: int, training: bool) -> bool:
    """A pass of this descriptor reads the MX region of the packed buffer (resr_pack_weights_mx fills it)."""
    return bool(plan & ((X2_PLAN_MX_BWD | X2_PLAN_MX_TRAIN_FORWARD) if training else X2_PLAN_MX_INFER))


def x2_plan_layout_key(plan: int) -> int:
    """The bits that size a workspace (the q tensors of the MX plans): workspaces of plans with equal keys are interchangeable."""
    return plan & (X2_PLAN_MX_INFER | X2_PLAN_MX_BWD | X2_PLAN_MX_WGRAD | X2_PLAN_MX_TAIL | X2_PLAN_MX_TRAIN_FORWARD)


def fetch_pack_table(call, what: str):
    """A native pack table as a host `PackChunk` array.  `call(chunks, capacity)` is the table function with its leading arguments
    bound: asked with (None, 0) for its length, then with an array of that length."""
    n = int(call(None, 0))
    if n <= 0:
        check(n if n < 0 else -1, what)
    host = (PackChunk * n)()
    got = int(call(C.cast(host, C.c_void_p), n))
    if got != n:
        check(got if got < 0 else -1, what)
    return host


def conv_pack_table(cout: int, cin: int, transposed: int = 0, src_off: int = 0, dst_off: int = 0, scale: float = 1.0):
    """The library's chunk table of one OIHW 3x3 convolution in one orientation (resr_conv_pack_table: the packed format is the
    library's alone, csrc/packed_layout.h) and the packed elements it takes from `dst_off` on."""
    host = fetch_pack_table(lambda chunks, n: lib().resr_conv_pack_table(cout, cin, transposed, src_off, dst_off, scale, chunks, n),
                            "resr_conv_pack_table")
    return host, int(lib().resr_conv_packed_elems(cout, cin))


def upload_chunks(chunks, device):
    """A `PackChunk` array as the device byte tensor resr_pack_weights reads."""
    import torch
    return torch.frombuffer(bytearray(bytes(chunks)), dtype=torch.uint8).to(device)


_lib = None


def lib() -> C.CDLL:
    """Load libresr_hip.so (built by csrc/build.py).  Raises if it is missing -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python real_esrgan-pytorch_amd/csrc/build.py` "
                "(or __graft_entry__.build()); the MI355X path has no CPU/PyTorch fallback")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.resr_version() != RESR_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {handle.resr_version()}, this package binds version {RESR_VERSION}: "
                               "rebuild it (python real_esrgan-pytorch_amd/csrc/build.py --force)")
        _lib = handle
    return _lib


def exported_symbols():
    return sorted(_PROTOS)


def check(rc: int, what: str = "resr") -> None:
    if rc != 0:
        msg = lib().resr_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def chain_health(sync: bool = False) -> None:
    """Raise if a chained dense-block launch (conv3x3_ws.h, CH) ever gave up waiting for a neighbouring tile or found
    an XCD with more than its share of workgroups (such a launch also poisons its output with NaNs, so a training loss
    shows it at once).  sync=False reads two host-mapped counters -- no synchronisation, cheap enough for every logging
    interval; sync=True drains the device first (end of an epoch / a benchmark)."""
    e = int(lib().resr_debug_chain_errors() if sync else lib().resr_chain_errors())
    if e != 0:
        raise RuntimeError(f"chained conv launches reported errors: {e & 0xffffffff} polls timed out, {e >> 32} workgroups beyond "
                           "their XCD's share (set RESR_CONV_NO_CHAIN=1 to run one launch per pass)")


def ptr(t):
    """Raw device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(ref=None):
    """The HIP stream a call should be enqueued on: the current stream of the device that owns `ref` (a tensor), else of
    the current device.  The library switches to the stream's device itself (csrc/api.hip DeviceScope)."""
    import torch
    dev = ref.device if ref is not None and getattr(ref, "is_cuda", False) else None
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def require_cuda(t, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the MI355X device, got {t.device}; "
                           "this package has no CPU path (the CPU oracle lives under oracle/ for tests only)")
