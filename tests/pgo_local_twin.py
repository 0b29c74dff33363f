"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/pgo_local_twin.cpp, the host replay of the local-frame PGO solve.

``pgo_local_twin.cpp`` includes the header the kernel's local instantiations include (``mac-vo_amd/csrc/pgo_local_dev.h``) and wraps the existing
twin's solve (``pgo_twin.cpp``).  The CPU suite pins it to the reference golden, the GPU suite pins the kernel to it.  The product path never builds
or loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRCS = [os.path.join(ROOT, "tests", "c_abi", "pgo_local_twin.cpp"), os.path.join(ROOT, "tests", "c_abi", "pgo_twin.cpp"),
         os.path.join(ROOT, "mac-vo_amd", "csrc", "pgo_math.h"), os.path.join(ROOT, "mac-vo_amd", "csrc", "pgo_local_dev.h")]
_lib = None


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (one rounding per fp32 operation, fma() the one fused one) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    out_dir = os.path.join(tempfile.gettempdir(), f"macvo_pgo_twin_{os.getuid()}")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libpgo_local_twin.so")
    newest = max(os.path.getmtime(f) for f in _SRCS)
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        _SRCS[0], "-o", tmp, "-lm"], check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.pgo_local_twin_solve.restype = C.c_int
    return _lib


def solve(batch, ref_pose, graph_type: str = "disp", params=None, min_points: int = 0, nw: int = 0, spec: int = 1):
    """``ops.pgo_solve(..., ref_pose=...)`` on a CPU ``PGOBatch``: a namespace with ``pose`` [nprob,7] f64 (local frame), ``info`` [nprob,4] f64,
    ``pose_f32`` [nprob,7] (world) and the stages ``init_local`` [nprob,7] f32, ``pos_To`` [Ntot,3] f32, ``cov_To`` [Ntot,3,3] f64 (or None)."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = build()
    p = params or ops.lm_default_params()
    nprob = batch.init_pose.shape[0]
    ntot = batch.pos_Tw.shape[0]
    keep = []

    def ptr(t, dt):
        if t is None:
            return C.c_void_p(None)
        t = t.detach().to("cpu", dt).contiguous()
        keep.append(t)
        return C.c_void_p(t.data_ptr())

    valid = None if batch.valid is None else batch.valid.to(torch.uint8)
    out = SimpleNamespace(pose=torch.zeros((nprob, 7), dtype=torch.float64), info=torch.zeros((nprob, 4), dtype=torch.float64),
                          pose_f32=torch.zeros((nprob, 7), dtype=torch.float32), init_local=torch.zeros((nprob, 7), dtype=torch.float32),
                          pos_To=torch.zeros((ntot, 3), dtype=torch.float32),
                          cov_To=None if batch.cov_Tw is None else torch.zeros((ntot, 3, 3), dtype=torch.float64))
    gt = {"icp": L.MV_GRAPH_ICP, "reproj": L.MV_GRAPH_REPROJ, "disp": L.MV_GRAPH_DISP}[graph_type]
    rc = lib.pgo_local_twin_solve(
        C.c_int(nprob), ptr(batch.offsets, torch.int32), C.c_int(gt), ptr(batch.init_pose, torch.float32), ptr(ref_pose, torch.float32),
        ptr(batch.intrinsics, torch.float32), ptr(batch.baseline, torch.float32), ptr(batch.pos_Tw, torch.float32),
        ptr(batch.cov_Tw, torch.float64), ptr(batch.pixel2_uv, torch.float32), ptr(batch.pixel2_d, torch.float32),
        ptr(batch.pixel2_disp, torch.float32), ptr(batch.pixel2_disp_cov, torch.float32), ptr(batch.pixel2_uv_cov, torch.float32),
        ptr(batch.obs2_covTc, torch.float64), ptr(valid, torch.uint8), C.c_int(int(min_points)), C.byref(p),
        C.c_void_p(out.pose.data_ptr()), C.c_void_p(out.info.data_ptr()), C.c_void_p(out.pose_f32.data_ptr()), C.c_int(nw), C.c_int(spec),
        C.c_void_p(out.init_local.data_ptr()), C.c_void_p(out.pos_To.data_ptr()),
        C.c_void_p(None if out.cov_To is None else out.cov_To.data_ptr()))
    assert rc == 0, rc
    return out
