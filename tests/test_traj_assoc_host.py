"""CPU: the trajectory-association restatement (tests/traj_assoc_ref.py) checked on its own, the host twin of the two new kernels
(tests/c_abi/assoc_twin.cpp on mac-vo_amd/csrc/se3_interp.h) pinned to it, the gap to the reference's fp32 chain, and the bindings.

Measure (tests/traj_assoc_cases.pose_error): |got - ref| / s, s = max(1, track extent) for positions, 1 for quaternion components, each row up to a
common sign of its quaternion.  Flags and status are exact."""
import os
import re

import numpy as np
import pytest
import torch

from tests import assoc_twin as TW
from tests import traj_assoc_cases as AC
from tests import traj_assoc_ref as AR
from tests import traj_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------- (a) the restatement
def test_ref_ends_are_copies_with_flag():
    src, ts = TR.random_walk(20, 1), AC._clock(20, 2)
    tq = np.array([ts[0] - 1.0, ts[0], ts[-1], ts[-1] + 5.0])
    poses, flag, st = AR.ref64(src, ts, tq, rebase=False)
    assert st == "OK" and flag.tolist() == [1, 1, 1, 1]
    assert poses[:2].tobytes() == np.stack([src[0], src[0]]).tobytes() and poses[2:].tobytes() == np.stack([src[-1], src[-1]]).tobytes()


def test_ref_pure_translation_midpoint():
    src = np.array([[1.0, 2.0, 3.0, 0, 0, 0, 1.0], [3.0, -2.0, 7.0, 0, 0, 0, 1.0]])
    poses, flag, _ = AR.ref64(src, np.array([0.0, 2.0]), np.array([1.0]), rebase=False)
    assert flag.tolist() == [0]
    np.testing.assert_allclose(poses[0], [2.0, 0.0, 5.0, 0, 0, 0, 1.0], atol=1e-15)


def test_ref_pure_rotation_half_angle():
    a = 1.3
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    src = np.zeros((2, 7))
    src[0, 6] = 1.0
    src[1, 3:6], src[1, 6] = axis * np.sin(a / 2), np.cos(a / 2)
    poses, _, _ = AR.ref64(src, np.array([0.0, 1.0]), np.array([0.5]), rebase=False)
    np.testing.assert_allclose(poses[0, 3:6], axis * np.sin(a / 4), atol=1e-15)
    np.testing.assert_allclose(poses[0, 6], np.cos(a / 4), atol=1e-15)
    np.testing.assert_allclose(poses[0, :3], 0.0, atol=1e-15)


def test_ref_sign_flipped_quaternions_same_rotation():
    plain, flipped = AC.reference("quat_plain")[0], AC.reference("quat_alternating")[0]
    assert AC.pose_error(flipped, plain, 1.0) <= 1e-14
    assert (np.sign(flipped[:, 6]) != np.sign(plain[:, 6])).any()            # the sign does follow the source: the comparison up to sign is needed


def test_ref_single_pose_all_copies():
    c = AC.cases()["shape_T1_Q257"]
    poses, flag, st = AC.reference("shape_T1_Q257")
    assert st == "OK" and flag.all() and (poses == c.src[0]).all()


def test_ref_exact_interior_hit_is_not_flagged():
    for name in AC.OK_CASES:
        c = AC.cases()[name]
        if c.interior_hits is not None and len(c.interior_hits):
            assert not AC.reference(name)[1][c.interior_hits].any(), name
    assert sum(len(c.interior_hits) for c in AC.cases().values() if c.interior_hits is not None) > 100


def test_ref_origin_lands_on_reference_row():
    c = AC.cases()["origin"]
    poses, flag, _ = AC.reference("origin")
    want = np.array(c.origin)
    want[3:] = -want[3:] / np.linalg.norm(want[3:])                        # given with w < 0
    assert flag[0] == 1 and poses[0, 6] >= 0 and np.abs(poses[0] - want).max() <= 1e-14
    assert (poses[:, 6] >= -1e-15).all()
    assert AC.pose_error(AC.reference("origin_moved")[0], poses, AC.scale_of(c)) <= 1e-13


def test_ref_status_of_every_case():
    for name, c in AC.cases().items():
        poses, flag, st = AC.reference(name)
        assert st == c.status, name
        if st != "OK":
            assert np.isnan(poses).all() and not flag.any() and poses.shape == (len(c.tq), 7)


# ---------------------------------------------------------------------------------------------------------------------------- (b) the twin
def _twin(c, out_dtype=None):
    return TW.lane(c.src, c.ts, c.tq, c.origin, c.rebase, out_dtype)


@pytest.mark.parametrize("name", AC.OK_CASES)
def test_twin_matches_ref64(name):
    c = AC.cases()[name]
    want, wflag, _ = AC.reference(name)
    got, flag, st = _twin(c, np.float64)
    assert AR.STATUS[st] == "OK" and flag.tobytes() == wflag.tobytes()
    assert AC.pose_error(got, want, AC.scale_of(c)) <= AC.ASSOC_BOUND


def test_twin_worst_error():
    """The figure recorded as ASSOC_ERR_MEASURED."""
    worst = max((AC.pose_error(_twin(AC.cases()[n], np.float64)[0], AC.reference(n)[0], AC.scale_of(AC.cases()[n])), n) for n in AC.OK_CASES)
    print(f"ASSOC worst |twin - ref64| / s = {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= AC.ASSOC_BOUND and AC.ASSOC_ERR_MEASURED < 1e-9


@pytest.mark.parametrize("name", AC.BAD_CASES)
def test_twin_status(name):
    c = AC.cases()[name]
    got, flag, st = _twin(c, np.float64)
    assert AR.STATUS[st] == c.status and np.isnan(got).all() and not flag.any()


def test_twin_stride_and_copies():
    a, b = _twin(AC.cases()["stride9"]), _twin(AC.cases()["stride7"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = AC.cases()["f32_T40"]
    got, flag, _ = _twin(c)                                                 # fp32 in, fp32 out: a copy is the row itself
    assert got.dtype == np.float32
    ts, tq = AR.rebased(c.ts, c.rebase), AR.rebased(c.tq, c.rebase)
    assert (got[tq <= ts[0]] == c.src[0]).all() and (got[tq >= ts[-1]] == c.src[-1]).all() and flag[(tq <= ts[0]) | (tq >= ts[-1])].all()


def test_twin_int64_rebase_in_integers():
    """int64 stamps == fp64 stamps holding the exactly rebased differences (Python integers), bit for bit; converting first changes prop."""
    c = AC.cases()["int64"]
    ts_exact = np.array([float(int(x) - int(c.ts[0])) for x in c.ts])
    tq_exact = np.array([float(int(x) - int(c.tq[0])) for x in c.tq])
    a, b = _twin(c, np.float64), TW.lane(c.src, ts_exact, tq_exact, None, True, np.float64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == 0
    early = TW.lane(c.src, c.ts.astype(np.float64), c.tq.astype(np.float64), None, True, np.float64)      # astype(float) first: multiples of 256 ns
    assert early[0].tobytes() != a[0].tobytes()
    assert (c.ts % 256 != 0)[1:].all() and not np.array_equal(c.ts.astype(np.float64) - float(c.ts[0]), ts_exact)


def test_gap_to_the_reference_chain():
    """The figure recorded as ASSOC_F32_CHAIN_MEASURED: ref64 rounded once to fp32 against the reference's mixed fp32 / fp64 chain."""
    worst, n = 0.0, 0
    for name in AC.OK_CASES:
        c = AC.cases()[name]
        if c.src.dtype != np.float32:
            continue
        assert AR.max_segment_angle(c.src) < np.pi / 2
        chain, cflag = AR.ref_chain(c.src, c.ts, c.tq, c.origin, c.rebase)
        want, wflag, _ = AC.reference(name)
        assert chain.dtype == np.float32 and cflag.tobytes() == wflag.tobytes()
        worst = max(worst, AC.pose_error(want.astype(np.float32), chain, AC.scale_of(c)))
        n += 1
    print(f"ASSOC worst |ref64 as fp32 - ref_chain| / s = {worst:.3e} over {n} fp32 cases")
    assert n >= 4 and worst <= AC.ASSOC_F32_CHAIN_BOUND and AC.ASSOC_F32_CHAIN_MEASURED <= 1e-5


@pytest.mark.parametrize("T", AC.POSE_T)
@pytest.mark.parametrize("pattern", AC.POSE_PATTERNS)
def test_twin_pose_interpolate(T, pattern):
    pose, need, (want, want_need, want_mask) = AC.pose_case(T, pattern)
    got, got_need, mask = TW.pose_interpolate(pose, need)
    assert mask.tobytes() == want_mask.tobytes() and got_need.tobytes() == want_need.tobytes()
    good = mask == 0
    assert got[good].tobytes() == pose[good].tobytes()
    assert (np.abs(got[~good].astype(np.float64) - want[~good]) <= AC.ulp32(want[~good])).all()
    if T <= 10:
        assert not mask.any() and not got_need.any()
    if pattern == "all_inner" and T > 10:
        assert mask.sum() == T - 10


def test_twin_standalone_under_sanitizers():
    """The twin's own main as a stand-alone program with -fsanitize=address,undefined: host code only, nothing loaded into Python."""
    assert "assoc_twin: OK" in TW.run_standalone_sanitized()


# ---------------------------------------------------------------------------------------------------------------------------- (c) bindings
def test_assoc_symbols_declared_and_bound():
    import ctypes as C

    import macvo_amd._lib as L

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "macvo_hip.h")).read(), flags=re.S)
    for sym in ("mv_traj_associate_lanes", "mv_pose_interpolate", "mv_pose_interpolate_lanes"):
        assert re.search(r"\b%s\s*\(" % sym, src) and sym in L.SIGNATURES, sym
    assert int(re.search(r"MV_TRAJ_UNSORTED\s*=\s*(\d+)", src).group(1)) == L.MV_TRAJ_UNSORTED == 4
    body = re.search(r"enum\s*\{\s*(MV_TRAJ_TIME_F64.*?)\}", src).group(1)
    assert [int(x.split("=")[1]) for x in body.split(",")] == [L.MV_TRAJ_TIME_F64, L.MV_TRAJ_TIME_I64]
    assert L.TRAJ_ASSOC_STATUS == AR.STATUS and L.TRAJ_ASSOC_STATUS[L.MV_TRAJ_UNSORTED] == "UNSORTED" and L.TRAJ_ASSOC_STATUS[:4] == L.TRAJ_STATUS
    hdr = open(os.path.join(ROOT, "mac-vo_amd", "csrc", "se3_interp.h")).read()
    for fn in ("q_act", "q_mul", "se3_mul", "se3_inv", "se3_normq", "skew_sq_apply", "se3_log", "se3_exp", "load_pose", "se3_interp"):
        assert re.search(r"SE3_HD \w+ %s\(" % fn, hdr), fn
    vm = open(os.path.join(ROOT, "mac-vo_amd", "csrc", "visual_map.hip")).read()
    assert '#include "se3_interp.h"' in vm and "se3_log(const Se3d" not in vm
    lib = L.load()
    # refusals that need no device: argument checks come before the launch
    one = (C.c_void_p * 1)(8)
    n = (C.c_int32 * 1)(4)
    big = (C.c_int32 * 1)((1 << 20) + 1)
    call = lib.mv_traj_associate_lanes
    assert call(0, one, one, n, one, n, None, 0, 0, 0, 0, 7, 1, one, one, 8, None) == -1
    assert call(65, one, one, n, one, n, None, 0, 0, 0, 0, 7, 1, one, one, 8, None) == -1
    assert call(1, one, one, big, one, n, None, 0, 0, 0, 0, 7, 1, one, one, 8, None) == -1
    assert call(1, one, one, n, one, big, None, 0, 0, 0, 0, 7, 1, one, one, 8, None) == -1
    assert call(1, one, one, n, one, n, None, 2, 0, 0, 0, 7, 1, one, one, 8, None) == -1          # src dtype
    assert call(1, one, one, n, one, n, None, 0, 2, 0, 0, 7, 1, one, one, 8, None) == -1          # time dtype
    assert call(1, one, one, n, one, n, None, 0, 0, 0, 0, 6, 1, one, one, 8, None) == -1          # stride < 7
    assert call(1, one, one, n, one, n, None, 0, 0, 0, 0, 7, 1, one, one, None, None) == -1       # status
    assert lib.mv_pose_interpolate(None, None, 3, None, None) == -1
    assert lib.mv_pose_interpolate_lanes(8, 65, n, 8, 4, None) == -1
    assert lib.mv_pose_interpolate_lanes(8, 1, n, 8, 3, None) == -1                                # mask_stride < T


def test_postprocess_config_mapper():
    from types import SimpleNamespace

    from macvo_amd import pipeline as P

    assert P.postprocess_config_fields({"type": "MotionInterpolate", "args": {}}) == {"interpolate": "motion"}
    assert P.postprocess_config_fields(SimpleNamespace(type="PoseInterpolate", args=SimpleNamespace())) == {"interpolate": "pose"}
    with pytest.raises(ValueError, match="has no HIP form"):
        P.postprocess_config_fields({"type": "SplineInterpolate", "args": {}})
