"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/kp_grad_twin.cpp, the host replay of the image-gradient selector kernels.

``kp_grad_twin.cpp`` includes the kernels' own arithmetic header (``mac-vo_amd/csrc/kp_grad_math.h``) and replays the per-pixel gradient, the fixed-order
fp64 reduction with the kernels' tile geometry and the selection with g++.  The CPU suite pins it to the torch restatement (``tests/grad_selectors_ref.py``)
before the kernels reach a GPU; the GPU suite compares the kernels with it bit for bit.  The product path never builds or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "kp_grad_twin.cpp")
_HDRS = [os.path.join(ROOT, "mac-vo_amd", "csrc", "kp_grad_math.h")]
_lib = None


def _out_dir() -> str:
    d = os.path.join(tempfile.gettempdir(), f"macvo_kp_grad_twin_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per operation, as the library's own flags) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(_out_dir(), "libkp_grad_twin.so")
    newest = max(os.path.getmtime(f) for f in [_SRC] + _HDRS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", _SRC, "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.kp_grad_twin.restype = C.c_int
    _lib.kp_grad_twin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 5
    return _lib


def run_standalone_sanitized() -> str:
    """The twin's own ``main`` as a stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into Python)."""
    exe = os.path.join(_out_dir(), f"kp_grad_twin_asan.{os.getpid()}")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DKP_GRAD_TWIN_MAIN",
                    _SRC, "-o", exe, "-lm"], check=True)
    try:
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        os.remove(exe)


def select(image, mask_width: int, grad_std: float, nms_size: "int | None" = None) -> SimpleNamespace:
    """One image ``[3, H, W]`` fp32 (numpy or CPU torch) -> ``cand`` int32 [n] (v * W + u), ``n_above``, ``grad`` fp32 [H, W], ``stats`` fp32 (mean, std,
    thr) and ``sums`` fp64 (sum g, sum g^2): what the kernels leave in out_cand / out_count / the workspace plane / out_stats."""
    img = np.ascontiguousarray(np.asarray(image, dtype=np.float32))
    _, H, W = img.shape
    grad = np.zeros((H, W), np.float32)
    cand = np.zeros(H * W, np.int32)
    count = np.zeros(2, np.int32)
    stats = np.zeros(3, np.float32)
    sums = np.zeros(2, np.float64)
    rc = build().kp_grad_twin(img.ctypes.data, H, W, int(mask_width), int(nms_size or 0), float(grad_std), grad.ctypes.data, cand.ctypes.data,
                              count.ctypes.data, stats.ctypes.data, sums.ctypes.data)
    assert rc == 0, rc
    return SimpleNamespace(cand=cand[: count[0]].copy(), n_above=int(count[1]), grad=grad, stats=stats, sums=sums)
