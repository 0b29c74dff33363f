"""TEST INFRASTRUCTURE: the input cases of the trajectory-association and PoseInterpolate tests (CPU twin and GPU kernels share them), the error
measure both use, and the two measured constants.  Everything is built once, on the CPU, and never modified."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import traj_assoc_ref as AR
from tests import traj_ref as TR

# Worst |twin - ref64| / s over every OK case of this file (tests/test_traj_assoc_host.py::test_twin_worst_error prints it), s = max(1, track extent)
# for positions and 1 for quaternion components, compared up to a common sign.  Tests assert 8 x it (the margin convention of TRAJ_ERR_MEASURED: it
# covers a different libm and the device's transcendental functions).  It must stay under 1e-9: correct fp64 arithmetic sits orders of magnitude below.
ASSOC_ERR_MEASURED = 5.815e-16
ASSOC_BOUND = 8 * ASSOC_ERR_MEASURED
# Worst |ref64 rounded to fp32 - ref_chain| / s over the fp32 cases whose per-segment rotation is below 90 degrees
# (test_gap_to_the_reference_chain prints it): what the reference's mixed fp32 / fp64 chain differs by from fp64 arithmetic with one rounding.  Above
# 1e-5 (about 170 fp32 roundings of the extent) it would be a mistake, not rounding.
ASSOC_F32_CHAIN_MEASURED = 1.707e-7
ASSOC_F32_CHAIN_BOUND = 8 * ASSOC_F32_CHAIN_MEASURED
assert ASSOC_ERR_MEASURED < 1e-9 and ASSOC_F32_CHAIN_MEASURED <= 1e-5

SHAPE_T = (1, 2, 3, 1024, 1025)
SHAPE_Q = (1, 255, 256, 257, 1000)
EUROC_T0 = 1403636579763555584                                     # a EuRoC nanosecond stamp: not representable in fp64 beyond multiples of 256


@dataclass
class Case:
    name: str
    src: np.ndarray                     # [T, >= 7] fp32 / fp64
    ts: np.ndarray                      # [T] fp64 / int64
    tq: np.ndarray                      # [Q], the dtype of ts
    origin: np.ndarray | None = None    # [7] or None
    rebase: bool = False                # on: each clock relative to its OWN first element (the queries are shuffled, so their base is any of them)
    status: str = "OK"
    interior_hits: np.ndarray | None = None   # indices of the queries that lie exactly on an interior stamp (cases without rebase)


def _clock(T: int, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)
    return 100.0 + np.concatenate([[0.0], np.cumsum(g.uniform(0.05, 0.15, size=max(T - 1, 0)))])[:T]


def _queries(ts: np.ndarray, Q: int, seed: int):
    """Q stamps, shuffled, with duplicates: before and at ts[0], at and after ts[-1], exactly on interior stamps, the rest uniform inside.  The kinds
    cycle, so a small Q takes the first few."""
    g = np.random.default_rng(seed)
    T = len(ts)
    span = max(ts[-1] - ts[0], 1.0)
    kinds = []
    for k in range(Q):
        m = k % 8
        if m == 0 or m >= 6:
            kinds.append(g.uniform(ts[0], ts[0] + span) if T > 1 else ts[0] + g.uniform(-1, 1))
        elif m == 1:
            kinds.append(ts[0] - g.uniform(0.01, 1.0))
        elif m == 2:
            kinds.append(ts[0])
        elif m == 3:
            kinds.append(ts[-1])
        elif m == 4:
            kinds.append(ts[-1] + g.uniform(0.01, 1.0))
        else:
            kinds.append(ts[g.integers(1, T - 1)] if T > 2 else ts[0] + 0.5 * span)
    tq = np.array(kinds)
    if Q >= 8:
        tq[7::16] = tq[5::16][:len(tq[7::16])]                     # repeats
    tq = tq[g.permutation(Q)]
    hits = np.nonzero(np.isin(tq, ts[1:-1]))[0] if T > 2 else np.zeros(0, np.int64)
    return tq, hits


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rot_track(angles, axis=(0.0, 0.0, 1.0)) -> np.ndarray:
    """Poses rotating about one axis by the given absolute angles (rad), positions on a slow line."""
    axis = _unit(axis)
    out = np.zeros((len(angles), 7))
    for i, a in enumerate(angles):
        out[i, :3] = (0.2 * i, -0.1 * i, 0.05 * i)
        out[i, 3:6] = axis * np.sin(0.5 * a)
        out[i, 6] = np.cos(0.5 * a)
    return out


@functools.lru_cache(maxsize=None)
def cases() -> "dict[str, Case]":
    out: dict = {}

    def add(c: Case):
        assert c.name not in out
        for a in (c.src, c.ts, c.tq, c.origin):
            if a is not None:
                a.setflags(write=False)
        out[c.name] = c

    # 1. shapes: fp64 rows, fp64 stamps
    for T in SHAPE_T:
        src, ts = TR.random_walk(T, 100 + T), _clock(T, 200 + T)
        for Q in SHAPE_Q:
            tq, hits = _queries(ts, Q, 1000 * T + Q)
            add(Case(f"shape_T{T}_Q{Q}", src.copy(), ts.copy(), tq, interior_hits=hits))
    # 2. a [T, 9] table: a row stride above 7, the spare columns must not be read
    src, ts = TR.random_walk(130, 31), _clock(130, 32)
    wide = np.full((130, 9), 1.0e30)
    wide[:, :7] = src
    tq, hits = _queries(ts, 300, 33)
    add(Case("stride9", wide, ts, tq, interior_hits=hits))
    add(Case("stride7", src.copy(), ts.copy(), tq.copy(), interior_hits=hits))
    # 3. int64 nanosecond stamps: 20 Hz with odd offsets that are not multiples of 256
    T = 200
    g = np.random.default_rng(41)
    its = EUROC_T0 + np.arange(T, dtype=np.int64) * 50_000_000 + np.concatenate([[0], 2 * g.integers(0, 5000, size=T - 1) + 1]).astype(np.int64)
    itq = EUROC_T0 - 777 + np.sort(g.integers(0, 50_000_000 * T, size=333)).astype(np.int64) | 1
    itq[5], itq[6] = its[17], its[100]
    add(Case("int64", TR.random_walk(T, 42), its, itq, rebase=True))
    # 4. fp32 in (fp32 out is the caller's choice)
    for T, Q, seed in ((1360, 4000, 51), (40, 257, 52)):
        src, ts = TR.random_walk(T, seed).astype(np.float32), _clock(T, seed + 1)
        tq, hits = _queries(ts, Q, seed + 2)
        add(Case(f"f32_T{T}", src, ts, tq, interior_hits=hits))
        add(Case(f"f32_T{T}_origin", src.copy(), ts.copy(), tq.copy(), origin=np.array([3.0, -2.0, 1.0, *(_unit([0.1, -0.2, 0.3, 0.9]))]), rebase=True))
    # 5. rotation branches
    ts5 = np.arange(6, dtype=np.float64)
    tq5 = np.array([0.5, 1.25, 2.5, 3.0, 3.75, 4.5, 2.0, 0.0, 5.0, 1.0 + 1e-3])
    half = np.zeros((6, 7))
    half[:, 6] = 1.0
    half[1::2, 3:] = (1.0, 0.0, 0.0, 0.0)                            # every segment exactly 180 degrees: q_e q_s^-1 has w == 0
    half[:, 0] = np.arange(6) * 0.5
    add(Case("rot_180", half, ts5, tq5))
    a = np.deg2rad(179.999)
    add(Case("rot_179_999", _rot_track([0, a, 2 * a, 3 * a, 4 * a, 5 * a], (1, 2, -2)), ts5.copy(), tq5.copy()))
    add(Case("rot_tiny", _rot_track(np.arange(6) * 3e-10, (2, -1, 2)), ts5.copy(), tq5.copy()))
    add(Case("rot_zero", _rot_track(np.zeros(6)), ts5.copy(), tq5.copy()))
    alt = TR.random_walk(60, 61)
    alt[1::2, 3:] *= -1.0
    tq, hits = _queries(_clock(60, 62), 200, 63)
    add(Case("quat_alternating", alt, _clock(60, 62), tq, interior_hits=hits))
    add(Case("quat_plain", TR.random_walk(60, 61), _clock(60, 62), tq.copy(), interior_hits=hits))
    # 6. status
    src, ts = TR.random_walk(50, 71), _clock(50, 72)
    tq, _ = _queries(ts, 100, 73)
    bad = ts.copy()
    bad[20], bad[21] = ts[21], ts[20]
    add(Case("bad_unsorted", src.copy(), bad, tq.copy(), status="UNSORTED"))
    bad = ts.copy()
    bad[30] = bad[29]
    add(Case("bad_equal", src.copy(), bad, tq.copy(), status="UNSORTED"))
    add(Case("bad_T0", src[:0].copy(), ts[:0].copy(), tq.copy(), status="TOO_SHORT"))
    bad = ts.copy()
    bad[7] = np.nan
    add(Case("bad_nan_stamp", src.copy(), bad, tq.copy(), status="NONFINITE"))
    bad = src.copy()
    bad[49, 4] = np.inf
    add(Case("bad_inf_pose", bad, ts.copy(), tq.copy(), status="NONFINITE"))
    bad = tq.copy()
    bad[99] = -np.inf
    add(Case("bad_inf_query", src.copy(), ts.copy(), bad, status="NONFINITE"))
    add(Case("bad_nan_origin", src.copy(), ts.copy(), tq.copy(), origin=np.array([0, 0, np.nan, 0, 0, 0, 1.0]), status="NONFINITE"))
    add(Case("good_a", src.copy(), ts.copy(), tq.copy()))
    add(Case("good_b", TR.random_walk(300, 74), _clock(300, 75), _queries(_clock(300, 75), 257, 76)[0]))
    # 7. origin
    ref0 = np.array([10.0, -4.0, 2.5, *(-_unit([0.3, 0.1, -0.2, 0.7]))])          # w < 0 as given: the output must come with w >= 0
    src, ts = TR.random_walk(80, 81), _clock(80, 82)
    src = TR.rigid(src, [0.2, -0.4, 0.1], [1.0, 2.0, 3.0])
    tq = np.concatenate([[ts[0]], _queries(ts, 150, 83)[0]])
    add(Case("origin", src, ts, tq, origin=ref0, rebase=True))                      # tq[0] = ts[0]: both clocks rebase to the same instant
    add(Case("origin_moved", TR.rigid(src, [-1.1, 0.3, 0.8], [-30.0, 12.0, 7.0]), ts.copy(), tq.copy(), origin=ref0.copy(), rebase=True))
    return out


OK_CASES = [n for n, c in cases().items() if c.status == "OK"]
BAD_CASES = [n for n, c in cases().items() if c.status != "OK"]


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """``ref64`` of a case (computed once, shared, read-only)."""
    c = cases()[name]
    poses, flag, st = AR.ref64(c.src, c.ts, c.tq, c.origin, c.rebase)
    poses.setflags(write=False)
    flag.setflags(write=False)
    return poses, flag, st


def extent(poses: np.ndarray) -> float:
    p = np.asarray(poses, np.float64)[:, :3]
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0))) if len(p) else 0.0


def scale_of(c: Case) -> float:
    """s for positions: max(1, the extent of the source track as the placement sees it — after the origin alignment)."""
    src = np.asarray(c.src[:, :7], np.float64)
    if c.origin is not None and len(src):
        import torch

        src = AR.align_origin(torch.from_numpy(src.copy()), torch.from_numpy(np.asarray(c.origin[:7], np.float64).copy())).numpy()
    return max(1.0, extent(src))


def pose_error(got: np.ndarray, ref: np.ndarray, s: float) -> float:
    """Worst |got - ref| / s over positions (s) and quaternion components (1), each row compared up to a common sign of its quaternion."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    if got.shape[0] == 0:
        return 0.0
    assert np.isfinite(got).all()
    ep = np.abs(got[:, :3] - ref[:, :3]).max() / s
    eq = np.minimum(np.abs(got[:, 3:] - ref[:, 3:]).max(axis=1), np.abs(got[:, 3:] + ref[:, 3:]).max(axis=1)).max()
    return float(max(ep, eq))


# ------------------------------------------------------------------------------------------------ PoseInterpolate
POSE_T = (9, 10, 11, 12, 64, 300)
POSE_PATTERNS = ("none", "row5", "all_inner", "alternating", "edges")


def pose_flags(T: int, pattern: str) -> np.ndarray:
    f = np.zeros(T, np.uint8)
    if pattern == "row5":
        if T > 5:
            f[5] = 1
    elif pattern == "all_inner":
        f[5:max(T - 5, 5)] = 1
    elif pattern == "alternating":
        f[1::2] = 1
    elif pattern == "edges":
        f[:5] = 1
        f[-5:] = 1
        f[T // 2] = 1
    else:
        assert pattern == "none"
    return f


@functools.lru_cache(maxsize=None)
def pose_case(T: int, pattern: str):
    """-> (pose fp32 [T, 7], need_interp uint8 [T], (restated poses fp64, flags after, mask))."""
    pose = TR.random_walk(T, 900 + T).astype(np.float32)
    need = pose_flags(T, pattern)
    ref = AR.pose_interpolate(pose, need)
    for a in (pose, need) + ref:
        a.setflags(write=False)
    return pose, need, ref


def ulp32(x: np.ndarray) -> np.ndarray:
    """One fp32 ulp at |x|, as the issue writes it: 2^-23 max(1, |x|)."""
    return 2.0 ** -23 * np.maximum(1.0, np.abs(x))
