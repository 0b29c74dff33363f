"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/traj_twin.cpp, the host replay of the trajectory-evaluation kernel.

``traj_twin.cpp`` includes the kernel's own arithmetic header (``mac-vo_amd/csrc/traj_math.h``) and replays one lane with the kernel's reduction
order, with g++.  The CPU suite pins it to ``tests/traj_ref.py`` (the SVD, the reflection branch, the degenerate rule) before the kernel reaches a
GPU.  The product path never builds or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "traj_twin.cpp")
_HDRS = [os.path.join(ROOT, "mac-vo_amd", "csrc", "traj_math.h"), os.path.join(ROOT, "include", "macvo_hip.h")]    # everything the twin compiles
_lib = None


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per operation, as the library's own flags) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    out_dir = os.path.join(tempfile.gettempdir(), f"macvo_traj_twin_{os.getuid()}")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libtraj_twin.so")
    newest = max(os.path.getmtime(f) for f in [_SRC] + _HDRS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        _SRC, "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.traj_twin_lane.restype = C.c_int
    _lib.traj_twin_lane.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int64]
    _lib.traj_twin_svd3.restype = None
    _lib.traj_twin_svd3.argtypes = [C.c_void_p] * 4
    return _lib


def lane(est: np.ndarray, ref: np.ndarray, align: str = "umeyama", correct_scale: bool = False):
    """One lane as the kernel runs it: ``est`` / ``ref`` ``[T, >= 7]`` fp32 or fp64 numpy arrays (row stride = their second dimension)
    -> (row ``[len(EVAL_TRAJ_COLS)]`` fp64, err ``[4, T]`` fp64, NaN where nothing is written)."""
    from macvo_amd import _lib as L

    lib = build()
    est, ref = np.ascontiguousarray(est), np.ascontiguousarray(ref)
    assert est.dtype in (np.float32, np.float64) and ref.dtype in (np.float32, np.float64)
    assert est.ndim == 2 and ref.ndim == 2 and est.shape[0] == ref.shape[0]
    T = est.shape[0]
    row = np.full(len(L.EVAL_TRAJ_COLS), np.nan)
    err = np.full((4, max(T, 1)), np.nan)
    rc = lib.traj_twin_lane(est.ctypes.data, ref.ctypes.data, T, int(est.dtype == np.float64), int(ref.dtype == np.float64), max(est.shape[1], 7),
                            max(ref.shape[1], 7), L.TRAJ_ALIGN[align], int(correct_scale), row.ctypes.data, err.ctypes.data, err.shape[1])
    assert rc == 0, rc
    return row, err[:, :T]


def svd3(Cm: np.ndarray):
    """``traj::svd3``: -> (U, d, V) with ``Cm = U diag(d) V^T``."""
    lib = build()
    Cm = np.ascontiguousarray(Cm, np.float64)
    U, d, V = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
    lib.traj_twin_svd3(Cm.ctypes.data, U.ctypes.data, d.ctypes.data, V.ctypes.data)
    return U, d, V
