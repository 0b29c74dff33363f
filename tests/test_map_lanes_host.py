"""CPU: the host side of one device-resident map per lane of a batched pipe — ``stack_lanes`` carries every lane's timestamp, the lane entry points
exist with the argument types ``_lib.py`` declares (and refuse bad arguments before any launch), ``NativeHotPath.attach_maps`` checks its arguments."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mv_map_append_lanes", "mv_map_append_skipped_lanes", "mv_map_set_pose_lanes", "mv_frame_pipe_map_append_lanes", "mv_frame_pipe_map_skip_lanes")


def _frame(t):
    from macvo_amd.pipeline import FrameInputs

    z = torch.zeros
    return FrameInputs(fmap1=z(2, 4, 3, 4), fmap2=z(2, 4, 3, 4), coords=z(1, 2, 2, 3, 4), flow=z(2, 2, 24, 32), logcov=z(2, 2, 24, 32), time_ns=t)


def test_stack_lanes_carries_every_lanes_timestamp():
    from macvo_amd.pipeline import stack_lanes

    x = stack_lanes([_frame(700), _frame(11), _frame(123456789012345)])
    assert x.time_ns == 700                                     # still lane 0's: nothing that reads it changes
    assert x.lane_time_ns == [700, 11, 123456789012345]
    assert x.fmap1.shape[0] == 6 and x.coords.shape[1] == 6
    assert stack_lanes([_frame(5)]).lane_time_ns == [5]
    assert _frame(9).lane_time_ns is None                      # a plain frame: one timestamp for every lane


def test_lane_entry_points_resolve_with_their_declared_types():
    from macvo_amd import _lib as L

    lib = L.load()
    assert lib.mv_abi_version() == L.ABI_VERSION == 8          # appended entry points: the ABI version and every existing struct stay
    header = open(os.path.join(ROOT, "include", "macvo_hip.h")).read()
    P = C.c_void_p
    want = {
        "mv_map_append_lanes": [C.POINTER(L.mvMapFrameLanes), P, P],
        "mv_map_append_skipped_lanes": [P, C.c_int, P, P, P, C.c_float, P, P],
        "mv_map_set_pose_lanes": [P, C.c_int, C.c_int, P, P],
        "mv_frame_pipe_map_append_lanes": [P, P, C.c_int, C.c_int, P, P, C.c_float, P],
        "mv_frame_pipe_map_skip_lanes": [P, P, C.c_int, P, P, C.c_float, P],
    }
    assert sorted(want) == sorted(NEW)
    for sym in NEW:
        fn = getattr(lib, sym)
        assert fn.restype is C.c_int and list(fn.argtypes) == want[sym] == L.SIGNATURES[sym][1], sym
        assert f" {sym}(" in header, sym
    # the host struct: four int32, sixteen pointers, one float (the header's field order)
    names = [n for n, _ in L.mvMapFrameLanes._fields_]
    assert names == ["lanes", "cap", "prev_frame", "min_num_point", "n_rows", "time_ns", "valid", "kp0", "kp1", "vals", "sigma0", "sigma1", "cov0", "cov1",
                     "pos_Tw", "cov0_world", "color", "K", "T_BS", "prior_pose", "baseline"]
    assert C.sizeof(L.mvMapFrameLanes) == 16 + 16 * 8 + 8
    assert C.sizeof(L.mvMapStores) == 33 * 8 + 8 + 3 * 8 + 3 * 8 + 8   # unchanged: the device descriptor array is mvMapStores[lanes]
    # bad arguments are refused on the host, before any launch
    assert lib.mv_map_append_lanes(None, None, None) != L.MV_OK
    n_rows, times = (C.c_int32 * 2)(0, 5), (C.c_int64 * 2)(1, 2)
    fr = L.mvMapFrameLanes(lanes=2, cap=4, prev_frame=-1, min_num_point=10, n_rows=C.cast(n_rows, P), time_ns=C.cast(times, P), K=8, T_BS=8, baseline=0.25)
    assert lib.mv_map_append_lanes(C.byref(fr), None, None) != L.MV_OK            # no descriptor array
    assert lib.mv_map_append_lanes(C.byref(fr), 8, None) != L.MV_OK               # a lane with more rows than the tables hold
    n_rows[1] = 3
    assert lib.mv_map_append_lanes(C.byref(fr), 8, None) != L.MV_OK               # rows, but no tables
    fr.lanes = L.MV_MAX_LANES + 1
    assert lib.mv_map_append_lanes(C.byref(fr), 8, None) != L.MV_OK
    assert lib.mv_map_append_skipped_lanes(8, 0, 8, 8, 8, 0.25, C.cast(times, P), None) != L.MV_OK
    assert lib.mv_map_append_skipped_lanes(8, 2, 8, 8, 8, 0.25, None, None) != L.MV_OK
    assert lib.mv_map_set_pose_lanes(8, 2, -1, 8, None) != L.MV_OK
    assert lib.mv_map_set_pose_lanes(None, 2, 0, 8, None) != L.MV_OK
    assert lib.mv_frame_pipe_map_append_lanes(None, 8, 1, 0, 8, 8, 0.25, C.cast(times, P)) != L.MV_OK
    assert lib.mv_frame_pipe_map_skip_lanes(None, 8, 1, 8, 8, 0.25, C.cast(times, P)) != L.MV_OK


def test_attach_maps_checks_its_arguments():
    from macvo_amd import _lib as L
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam = Camera(320.0, 320.0, 128.0, 96.0, 0.25, 192, 256)
    K = torch.eye(3)
    hot = NativeHotPath(cam, HotPathConfig(), lanes=3)
    m = lambda n: NS(n_frames=n, last_keyframe=n - 1)  # noqa: E731  (what the checks look at, before anything touches the device)
    with pytest.raises(L.MacvoHipError, match=r"2 map\(s\) for 3 lane\(s\)"):
        hot.attach_maps([m(0), m(0)], K)
    with pytest.raises(L.MacvoHipError, match=r"4 map\(s\) for 3 lane\(s\)"):
        hot.attach_maps([m(0)] * 4, K)
    with pytest.raises(L.MacvoHipError, match="same number of frames"):
        hot.attach_maps([m(0), m(2), m(0)], K)
    with pytest.raises(L.MacvoHipError, match="one map per pipe, lanes must be 1"):
        hot.attach_map(m(0), K)                                                    # the one-map call stays one lane
    with pytest.raises(L.MacvoHipError, match=r"runs one sequence per pipe \(lanes == 1\)"):
        NativeHotPath(cam, HotPathConfig(mapping=True), lanes=2)                   # the dense-mapping tail stays one lane per pipe
    one = NativeHotPath(cam, HotPathConfig(mapping=True), lanes=1)
    with pytest.raises(L.MacvoHipError, match="attach_map"):
        one.attach_maps([m(0)], K)                                                 # ... and registers through attach_map
