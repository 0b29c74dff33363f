"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/resample_twin.cpp, the host replay of the frame resampler's index and weight arithmetic.

``resample_twin.cpp`` includes the kernels' own arithmetic header (``mac-vo_amd/csrc/resample_math.h``) and runs its functions with g++.  The CPU suite pins it
to torch and to the fp64 formula of ``tests/preprocess_ref.py`` before the kernels reach a GPU.  The product path never builds or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "resample_twin.cpp")
_HDRS = [os.path.join(ROOT, "mac-vo_amd", "csrc", "resample_math.h")]
_lib = None


def _out_dir() -> str:
    d = os.path.join(tempfile.gettempdir(), f"macvo_resample_twin_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per operation, as the library's own flags) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(_out_dir(), "libresample_twin.so")
    newest = max(os.path.getmtime(f) for f in [_SRC] + _HDRS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.resample_twin_nearest.restype = None
    _lib.resample_twin_nearest.argtypes = [C.c_int, C.c_int, C.c_void_p]
    _lib.resample_twin_aa.restype = None
    _lib.resample_twin_aa.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def run_standalone_sanitized() -> str:
    """The twin's own ``main`` as a stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into Python)."""
    exe = os.path.join(_out_dir(), f"resample_twin_asan.{os.getpid()}")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRESAMPLE_TWIN_MAIN",
                    _SRC, "-o", exe, "-lm"], check=True)
    try:
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        os.remove(exe)


def max_taps() -> int:
    return build().resample_twin_max_taps()


def nearest(n_in: int, n_out: int) -> np.ndarray:
    idx = np.zeros(n_out, np.int32)
    build().resample_twin_nearest(n_in, n_out, idx.ctypes.data)
    return idx


def aa(n_in: int, n_out: int, cap: int = 64):
    """-> (xmin [out], xsize [out], weights [out, cap] fp32, zero past each element's xsize)."""
    xmin, xsize = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    w = np.zeros((n_out, cap), np.float32)
    build().resample_twin_aa(n_in, n_out, cap, xmin.ctypes.data, xsize.ctypes.data, w.ctypes.data)
    return xmin, xsize, w
