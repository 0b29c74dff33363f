"""TEST INFRASTRUCTURE: builds and calls tests/c_abi/posenet_twin.cpp, the host replay of the PoseNet kernels, and holds what the CPU and
GPU PoseNet tests share: the seeded cases with their fp64 / fp32 torch references (computed once per process) and the error measure.

``posenet_twin.cpp`` includes the kernels' plan header (``mac-vo_amd/csrc/posenet_math.h``) and reads the buffer ``mv_posenet_pack`` wrote.
The product path never builds or loads it."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "c_abi", "posenet_twin.cpp")
_HDR = os.path.join(ROOT, "mac-vo_amd", "csrc", "posenet_math.h")
_lib = None

WEIGHT_SEEDS = (11, 12)
INPUT_SEED = 5
TOL_FACTOR = 16.0      # E(kernel or twin) <= 16 * E(torch's fp32 CPU forward of the same case): fp32 evaluations that differ in summation order


def build() -> C.CDLL:
    """g++ -O2 -ffp-contract=off (fmaf stays the one fused operation, nothing else is contracted) into a scratch directory."""
    global _lib
    if _lib is not None:
        return _lib
    out_dir = os.path.join(tempfile.gettempdir(), f"macvo_posenet_twin_{os.getuid()}")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libposenet_twin.so")
    newest = max(os.path.getmtime(_SRC), os.path.getmtime(_HDR))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.dirname(_HDR), _SRC, "-o", tmp, "-lm"],
                       check=True)
        os.replace(tmp, so)
    _lib = C.CDLL(so)
    _lib.posenet_twin_forward.restype = C.c_int
    _lib.posenet_twin_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    return _lib


def pack(sd) -> torch.Tensor:
    """``mv_posenet_pack`` of a bare-key state dict -> the packed fp32 host buffer."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = L.load()
    tensors = [sd[k].detach().to("cpu", torch.float32).contiguous() for k, _ in ops.posenet_tensor_table()]
    ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    packed = torch.empty((lib.mv_posenet_packed_bytes() // 4,), dtype=torch.float32)
    L.check(lib.mv_posenet_pack(ptrs, packed.data_ptr()), "mv_posenet_pack")
    return packed


def forward(packed: torch.Tensor, x: torch.Tensor):
    """(out [lanes,6], six stage tensors) of the host replay."""
    from macvo_amd import ops

    lib = build()
    x = x.detach().to("cpu", torch.float32).contiguous()
    lanes = x.shape[0]
    out = torch.zeros((lanes, 6), dtype=torch.float32)
    stages = [torch.zeros((lanes,) + s, dtype=torch.float32) for s in ops.POSENET_STAGE_SHAPES]
    sp = (C.c_void_p * 6)(*[s.data_ptr() for s in stages])
    rc = lib.posenet_twin_forward(packed.data_ptr(), x.data_ptr(), lanes, out.data_ptr(), sp)
    assert rc == 0, rc
    return out, stages


def rel_err(y: torch.Tensor, y64: torch.Tensor) -> float:
    """E(y) = max|y - y64| / max|y64|."""
    return float((y.detach().cpu().double() - y64).abs().max() / y64.abs().max())


@functools.lru_cache(maxsize=None)
def case(seed: int, lanes: int = 3):
    """A seeded case, computed once and shared (treat as read-only): state dict, input ``[lanes,5,112,160]``, the fp64 restatement's
    (out, stages) and, per tensor, the error E of torch's fp32 CPU forward against it — the tolerance's yardstick."""
    from tools import posenet_torch as PT

    sd = PT.seeded_state_dict(seed)
    x = PT.sample_input(3, INPUT_SEED)[:lanes].contiguous()
    with torch.no_grad():
        y64, st64 = PT.from_state_dict(sd, dtype=torch.float64)(x.double(), return_stages=True)
        y32, st32 = PT.from_state_dict(sd)(x, return_stages=True)
    e32 = [rel_err(y32, y64)] + [rel_err(a, b) for a, b in zip(st32, st64)]
    return sd, x, y64, st64, e32


def check_against_fp64(what: str, y, stages, ref, lanes=None) -> "list[float]":
    """Asserts E <= 16 * E(torch fp32 CPU) on the output and on every stage; returns the measured E (output first).  ``lanes``: the lane
    indices of the case that ``y`` / ``stages`` hold (default: the first ``y.shape[0]``)."""
    _, _, y64, st64, e32 = ref
    sel = slice(0, y.shape[0]) if lanes is None else lanes
    errs = [rel_err(y, y64[sel])] + [rel_err(a, b[sel]) for a, b in zip(stages, st64)]
    names = ("out", "firstconv", "layer1", "layer2", "layer3", "layer4", "layer5")
    print(f"[posenet] {what}: " + ", ".join(f"{n} E={e:.2e} (torch fp32 {r:.2e})" for n, e, r in zip(names, errs, e32)))
    for n, e, r in zip(names, errs, e32):
        assert e <= TOL_FACTOR * r, f"{what}: {n} is {e:.3e} of max|y64| from the fp64 restatement; the bar is 16 x {r:.3e} (torch's fp32 CPU forward)"
    return errs
