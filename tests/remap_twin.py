"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/remap_twin.cpp, the host replay of the remap kernel's per-pixel arithmetic.

``remap_twin.cpp`` includes the kernel's own arithmetic header (``mac-vo_amd/csrc/remap_math.h``) and runs its functions with g++.  The CPU suite pins it to the
numpy integer formula of ``tests/rectify_ref.py`` before the kernel reaches a GPU; the GPU suite compares the kernel with it bit for bit.  The product path never
builds or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "remap_twin.cpp")
_HDRS = [os.path.join(ROOT, "mac-vo_amd", "csrc", "remap_math.h")]
_lib = None


def _out_dir() -> str:
    d = os.path.join(tempfile.gettempdir(), f"macvo_remap_twin_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per operation, as the library's own flags) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(_out_dir(), "libremap_twin.so")
    newest = max(os.path.getmtime(f) for f in [_SRC] + _HDRS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.remap_twin_u8.restype = None
    _lib.remap_twin_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    _lib.remap_twin_unit.restype = None
    _lib.remap_twin_unit.argtypes = [C.c_void_p]
    _lib.remap_twin_quantise.restype = C.c_int
    _lib.remap_twin_quantise.argtypes = [C.c_float, C.POINTER(C.c_int32)]
    return _lib


def run_standalone_sanitized() -> str:
    """The twin's own ``main`` as a stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into Python)."""
    exe = os.path.join(_out_dir(), f"remap_twin_asan.{os.getpid()}")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DREMAP_TWIN_MAIN",
                    _SRC, "-o", exe, "-lm"], check=True)
    try:
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        os.remove(exe)


def remap_u8(src: np.ndarray, map_x: np.ndarray, map_y: np.ndarray, layout: str = "hwc", reverse: bool = False) -> np.ndarray:
    """One image: src uint8 ``[H, W, C]`` / ``[H, W]`` (hwc) or ``[C, H, W]`` (planar), maps fp32 ``[h, w]`` -> uint8 planar ``[C, h, w]``."""
    src = np.ascontiguousarray(src, np.uint8)
    if layout == "hwc":
        src = src.reshape(src.shape[0], src.shape[1], -1)
        H, W, Cn = src.shape
    else:
        Cn, H, W = src.shape
    mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    oh, ow = mx.shape
    dst = np.zeros((Cn, oh, ow), np.uint8)
    build().remap_twin_u8(src.ctypes.data, H, W, Cn, int(layout == "hwc"), int(reverse), mx.ctypes.data, my.ctypes.data, oh, ow, dst.ctypes.data)
    return dst


def remap_lanes_u8(src: np.ndarray, map_x: np.ndarray, map_y: np.ndarray, layout: str = "hwc", reverse: bool = False) -> np.ndarray:
    """A batch: src ``[lanes, ...]``, maps ``[h, w]`` (shared) or ``[lanes, h, w]`` -> ``[lanes, C, h, w]``."""
    return np.stack([remap_u8(src[l], map_x if map_x.ndim == 2 else map_x[l], map_y if map_y.ndim == 2 else map_y[l], layout, reverse)
                     for l in range(src.shape[0])])


def unit_table() -> np.ndarray:
    out = np.zeros(256, np.float32)
    build().remap_twin_unit(out.ctypes.data)
    return out


def quantise(m: float):
    s = C.c_int32(0)
    ok = build().remap_twin_quantise(float(m), C.byref(s))
    return bool(ok), s.value
