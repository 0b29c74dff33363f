"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/assoc_twin.cpp, the host replay of one lane of the trajectory-association kernel and of the
PoseInterpolate kernel.

``assoc_twin.cpp`` includes the kernels' own arithmetic header (``mac-vo_amd/csrc/se3_interp.h``) and runs its per-lane functions with g++.  The CPU
suite pins it to ``tests/traj_assoc_ref.py`` before the kernels reach a GPU.  The product path never builds or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "assoc_twin.cpp")
_HDRS = [os.path.join(ROOT, "mac-vo_amd", "csrc", "se3_interp.h"), os.path.join(ROOT, "include", "macvo_hip.h")]    # everything the twin compiles
_lib = None


def _out_dir() -> str:
    d = os.path.join(tempfile.gettempdir(), f"macvo_assoc_twin_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per operation, as the library's own flags) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(_out_dir(), "libassoc_twin.so")
    newest = max(os.path.getmtime(f) for f in [_SRC] + _HDRS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        _SRC, "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.assoc_twin_lane.restype = C.c_int
    _lib.assoc_twin_lane.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int,
                                     C.c_void_p, C.c_void_p]
    _lib.pose_interp_twin_lane.restype = None
    _lib.pose_interp_twin_lane.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_void_p]
    return _lib


def run_standalone_sanitized() -> str:
    """The twin's own ``main`` as a stand-alone program under -fsanitize=address,undefined (host code only; nothing is loaded into Python)."""
    exe = os.path.join(_out_dir(), f"assoc_twin_asan.{os.getpid()}")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DASSOC_TWIN_MAIN",
                    "-I", os.path.join(ROOT, "include"), _SRC, "-o", exe, "-lm"], check=True)
    try:
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    finally:
        os.remove(exe)


def lane(src: np.ndarray, ts: np.ndarray, tq: np.ndarray, origin: np.ndarray | None = None, rebase: bool = True, out_dtype=None):
    """One lane as the kernel runs it: ``src`` ``[T, >= 7]`` fp32 / fp64, ``ts`` ``[T]`` and ``tq`` ``[Q]`` fp64 or int64 (one dtype), ``origin`` ``[7]``
    or None -> (poses ``[Q, 7]``, extrapolated uint8 ``[Q]``, status)."""
    lib = build()
    src, ts, tq = np.ascontiguousarray(src), np.ascontiguousarray(ts), np.ascontiguousarray(tq)
    assert src.dtype in (np.float32, np.float64) and ts.dtype == tq.dtype and ts.dtype in (np.float64, np.int64)
    assert src.ndim == 2 and ts.shape == (src.shape[0],) and tq.ndim == 1
    out_dtype = np.dtype(out_dtype or src.dtype)
    T, Q = src.shape[0], tq.shape[0]
    org = None if origin is None else np.ascontiguousarray(origin[:7])
    out = np.zeros((max(Q, 1), 7), out_dtype)
    flag = np.zeros(max(Q, 1), np.uint8)
    st = lib.assoc_twin_lane(src.ctypes.data, ts.ctypes.data, T, tq.ctypes.data, Q, None if org is None else org.ctypes.data, int(src.dtype == np.float64),
                             int(ts.dtype == np.int64), int(org is not None and org.dtype == np.float64), int(out_dtype == np.float64),
                             max(src.shape[1], 7), int(rebase), out.ctypes.data, flag.ctypes.data)
    return out[:Q], flag[:Q], st


def pose_interpolate(pose: np.ndarray, need_interp: np.ndarray):
    """``PoseInterpolate`` on copies of ``pose`` ``[T, 7]`` fp32 and ``need_interp`` ``[T]`` -> (pose, need_interp, mask)."""
    lib = build()
    pose = np.array(pose, np.float32, order="C")
    need = np.array(need_interp, np.uint8, order="C")
    mask = np.zeros(max(len(need), 1), np.uint8)
    lib.pose_interp_twin_lane(pose.ctypes.data, need.ctypes.data, len(need), mask.ctypes.data)
    return pose, need, mask[:len(need)]
