"""ctypes binding of the C-ABI HIP library (include/gemnet_hip.h).

There is deliberately NO fallback: if ``csrc/libgemnet_hip.so`` is missing or a call fails the
product path raises.  PyTorch is used only for device memory and streams: every entry point
receives raw device pointers + sizes + ``torch.cuda.current_stream()``.
"""
import ctypes
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GEMNET_HIP_LIB") or os.path.join(_HERE, "csrc", "libgemnet_hip.so")

_vp = ctypes.c_void_p

# Everything below comes from include/gemnet_hip.h, which _abi reads once per process: the integer constants (GN_OP_*,
# GN_CHAIN_MAX_OPS, GN_ANG_F16, ... under the header's names), the argument structs, and name -> argtypes of every function.
ABI = _abi.read()
globals().update(ABI.consts)
GemmArgs, ChainOp, ChainArgs = (ABI.structs[n] for n in ("gn_gemm_args", "gn_chain_op", "gn_chain_args"))
# gn_gemm_args travels as a ctypes struct (byref); every other struct pointer is an address (kernels.chain packs the block
# with `struct`, the device tables are tensors)
SIGNATURES = {name: [ctypes.POINTER(GemmArgs) if kind == "struct:gn_gemm_args" else ct for _, ct, kind in params]
              for name, (_, params) in ABI.funcs.items()}

_lib = None
# hbcheck.Recorder while a captured step is being checked for unordered memory accesses (debug tool, hbcheck.py): `ptr`
# reports the tensors handed to a launch, `load` returns a proxy that reports the launch itself.  None otherwise.
TRACE = None


def load():
    """Load the HIP library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib if TRACE is None else TRACE.proxy(_lib)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    # (no setters: since ABI 13 the arithmetic of the angle-form kernels is an argument of each launch —
    #  kernels.ANG_F16_MASK holds the read-only host configuration)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ABI.funcs[name][0]
    _lib = lib
    return lib if TRACE is None else TRACE.proxy(lib)      # (also on the load itself: the first launch is traced too)


def check(code, what):
    if code != 0:
        msg = load().gn_error_string(code)
        raise RuntimeError(f"{what} failed: hip error {code} ({msg.decode() if msg else '?'})")


def stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    if TRACE is not None:
        TRACE.touch(t)
    return _vp(t.data_ptr())


def addr(t):
    """Raw device address of a tensor (for argument blocks packed by hand); reported to the recorder like `ptr`."""
    if TRACE is not None:
        TRACE.touch(t)
    return t.data_ptr()


def note(reads=(), writes=()):
    """Operands of the next launch that live in a device-resident table (invisible in the argument list)."""
    if TRACE is not None:
        TRACE.note(reads, writes)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "gemnet_pytorch_amd ops run only on a HIP device (MI355X); got a CPU tensor. "
                "There is no CPU fallback — use the oracle in tests if you need a CPU result.")
