"""GPU: one device-resident map per lane of a batched pipe (csrc/visual_map.hip map_append_lanes_kernel / map_skip_lanes_kernel /
map_set_pose_lanes_kernel, devmap.DeviceVisualMaps, NativeHotPath.attach_maps).

* the lane kernel against ``oracle.visual_map.OracleVisualMap`` (pinned to the real ``VisualMap`` by tests/golden) and against the one-frame kernel on the
  same lane slices: 3 lanes (odd), 300 rows per lane (crosses the 256-row chunk), the value table in the pipe's ``[11, lanes, cap]`` layout, stores of
  different capacities that re-grow at different frames;
* refusal is per lane: a lane whose match store is one row short is refused (``counts[4]``), nothing of it is written, the other lanes are complete;
* the driver: every lane of a 3-lane pipe leaves, bit for bit, what a one-lane pipe with ``attach_map`` leaves for that lane's sequence;
* pipes without maps are unchanged, and ``attach_maps([m])`` on a one-lane pipe equals ``attach_map(m)``;
* the one-lane C entry points (``mv_frame_pipe_map_append`` / ``_map_skip``), called by hand, leave what ``attach_maps([m])`` leaves.

Every comparison is exact (``np.array_equal``): the kernels copy rows, nothing is rounded."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu

LANES, CAP = 3, 300
ROWS = {0: (0, 37, 300, 300), 1: (0, 300, 300, 300), 2: (0, 300, 300, 300)}     # rows handed to the kernel per lane and frame (frame 0: initialize)
LOST_FRAME = 2                                                                  # lane 1: every row of this frame masked -> lost track
INIT = (16, 400, 4096)                                                          # the lanes' stores start differently: 16 and 400 re-grow, at different frames


def _same(got, want, what):
    assert set(got) == set(want), what
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w, equal_nan=True), (what, k)


def _tables(seed=5, all_valid_lane1=False):
    """Four frames of synthetic tables in the pipe's layouts + per-lane metadata (CPU)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    frames = []
    for t in range(4):
        valid = torch.zeros(LANES, CAP, dtype=torch.uint8)
        valid[0, : ROWS[0][t]] = (torch.rand(ROWS[0][t], generator=g) < 0.8).to(torch.uint8)
        v1 = (torch.rand(ROWS[1][t], generator=g) < 0.6).to(torch.uint8)          # (always drawn: both forms see the same tables)
        valid[1, : ROWS[1][t]] = 1 if all_valid_lane1 else v1
        if t == LOST_FRAME and not all_valid_lane1:
            valid[1] = 0
        valid[2, : ROWS[2][t]] = 1                                                                # NULL-equivalent: keep all
        frames.append(dict(valid=valid, kp0=r(LANES, CAP, 2) * 100, kp1=r(LANES, CAP, 2) * 100, vals=r(11, LANES, CAP), sigma0=r(LANES, CAP, 3).abs(),
                           sigma1=r(LANES, CAP, 3).abs(), cov0=r(LANES, CAP, 3, 3).double(), cov1=r(LANES, CAP, 3, 3).double(), pos_Tw=r(LANES, CAP, 3),
                           cov0w=r(LANES, CAP, 3, 3).double(), prior=r(LANES, 7), opt=r(LANES, 7),
                           time_ns=[10_000_000_000 * (l + 1) + 33 * t for l in range(LANES)]))
    meta = dict(K=torch.tensor([[320.0, 0, 128], [0, 321.0, 96], [0, 0, 1]]), baseline=0.25, T_BS=r(LANES, 7),
                skip_pose=r(LANES, 7), skip_time=[10_000_000_000 * (l + 1) + 999 for l in range(LANES)])
    return frames, meta


def _oracle_skip(ora, meta, l):
    """push_keyframe(frame, pose, need_interp=True) of a non-keyframe (MACVO.py:177-179,339-348) on the oracle's lists: one frame row, empty edge rows."""
    ora.frames["K"].append(meta["K"].reshape(1, 3, 3).float())
    ora.frames["baseline"].append(torch.tensor([meta["baseline"]], dtype=torch.float32))
    ora.frames["pose"].append(meta["skip_pose"][l].reshape(1, 7).float())
    ora.frames["T_BS"].append(meta["T_BS"][l].reshape(1, 7).float())
    ora.frames["need_interp"].append(torch.tensor([True]))
    ora.frames["time_ns"].append(torch.tensor([meta["skip_time"][l]], dtype=torch.long))
    for ranges, num in ((ora.f2m_ranges, ora.f2m_num), (ora.f2map_ranges, ora.f2map_num)):
        ranges.append(torch.full((ora.max_frame_range, 2), -1, dtype=torch.long))
        num.append(0)


def _oracle_lane(frames, meta, l, n_frames=4, skip=True):
    from oracle import visual_map as VM

    ora = VM.OracleVisualMap()
    m = dict(K=meta["K"], T_BS=meta["T_BS"][l], baseline=meta["baseline"])
    for t, fr in enumerate(frames[:n_frames]):
        n = ROWS[l][t]
        d = dict(n=n, time_ns=fr["time_ns"][l], prior=fr["prior"][l])
        if n:
            d.update(valid=fr["valid"][l, :n].bool(), kp0=fr["kp0"][l, :n], kp1=fr["kp1"][l, :n], vals=fr["vals"][:, l, :n], sigma0=fr["sigma0"][l, :n],
                     sigma1=fr["sigma1"][l, :n], cov0=fr["cov0"][l, :n], cov1=fr["cov1"][l, :n], pos_Tw=fr["pos_Tw"][l, :n], cov0w=fr["cov0w"][l, :n], color=None)
        idx = ora.push_frame(m, d)
        ora.set_pose(idx, fr["opt"][l])
    if skip:
        _oracle_skip(ora, meta, l)
    return ora.serialize()


@pytest.fixture(scope="module")
def case():
    frames, meta = _tables()
    return frames, meta, [_oracle_lane(frames, meta, l) for l in range(LANES)]      # computed once, shared, never modified


def _lane_frame(L, fr, meta, dev, t, prev_frame, keep):
    """mvMapFrameLanes over the frame's tables as they lie on the device."""
    d = {k: fr[k].to(dev).contiguous() for k in ("valid", "kp0", "kp1", "vals", "sigma0", "sigma1", "cov0", "cov1", "pos_Tw", "cov0w", "prior")}
    n_rows = (C.c_int32 * LANES)(*[ROWS[l][t] for l in range(LANES)])
    times = (C.c_int64 * LANES)(*fr["time_ns"])
    Kd, Td = meta["K"].to(dev).contiguous(), meta["T_BS"].to(dev).contiguous()
    keep.append((d, n_rows, times, Kd, Td))
    p = lambda x: x.data_ptr()  # noqa: E731
    return L.mvMapFrameLanes(lanes=LANES, cap=CAP, prev_frame=prev_frame, min_num_point=10, n_rows=C.cast(n_rows, C.c_void_p), time_ns=C.cast(times, C.c_void_p),
                             valid=p(d["valid"]), kp0=p(d["kp0"]), kp1=p(d["kp1"]), vals=p(d["vals"]), sigma0=p(d["sigma0"]), sigma1=p(d["sigma1"]),
                             cov0=p(d["cov0"]), cov1=p(d["cov1"]), pos_Tw=p(d["pos_Tw"]), cov0_world=p(d["cov0w"]), color=None, K=p(Kd), T_BS=p(Td),
                             prior_pose=p(d["prior"]), baseline=meta["baseline"])


def test_lane_kernel_equals_the_oracle_and_the_one_frame_kernel(gpu, case):
    from macvo_amd import _lib as L
    from macvo_amd import ops
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps

    frames, meta, want = case
    mps = DeviceVisualMaps(LANES, gpu, init_size=list(INIT))
    assert [m.cap["match"] for m in mps] == list(INIT)
    keep = []
    for t, fr in enumerate(frames):
        n_rows = [ROWS[l][t] for l in range(LANES)]
        mps.push_frames(_lane_frame(L, fr, meta, gpu, t, t - 1, keep), n_rows)
        mps.set_poses(t, fr["opt"].to(gpu))
    mps.push_skipped(meta["K"], meta["T_BS"], meta["baseline"], meta["skip_time"], meta["skip_pose"])
    torch.cuda.synchronize()
    caps = [m.cap["match"] for m in mps]
    assert caps[0] > INIT[0] and caps[1] > INIT[1] and caps[2] == INIT[2]                                # two lanes re-grew (lane 0 three times), one never did
    got = mps.serialize()
    for l in range(LANES):
        _same(got[l], want[l], f"lane {l} vs oracle")
        assert got[l]["frames//need_interp"].tolist() == [False, False, l == 1, False, True], l          # lane 1's masked frame only; the skipped row
        assert int(mps[l].counts.cpu()[3]) == int(l == 1) and mps[l].n_frames == 5
    assert got[0]["match//pixel1_uv"].shape[0] < 637 and got[2]["match//pixel1_uv"].shape[0] == 900
    # ... and the existing one-frame kernels on the same lane slices
    for l in range(LANES):
        solo = DeviceVisualMap(gpu, init_size=INIT[l])
        for t, fr in enumerate(frames):
            n = ROWS[l][t]
            kw = dict(K=meta["K"], T_BS=meta["T_BS"][l], baseline=meta["baseline"], time_ns=fr["time_ns"][l], prior_pose=fr["prior"][l])
            if n:
                d = lambda k: fr[k][l, :n].to(gpu).contiguous()  # noqa: E731
                tr = ops.TrackedKeypoints(d("kp0"), d("kp1"), None, fr["vals"][:, l, :n].to(gpu).contiguous(), d("sigma0"), d("sigma1"))
                kw.update(tracked=tr, valid=None if l == 2 else d("valid"), cov0=d("cov0"), cov1=d("cov1"), pos_Tw=d("pos_Tw"), cov0_world=d("cov0w"))
            idx = solo.push_frame(**kw)
            solo.set_pose(idx, fr["opt"][l].to(gpu))
        solo.push_skipped(meta["K"], meta["T_BS"][l], meta["baseline"], meta["skip_time"][l], meta["skip_pose"][l])
        torch.cuda.synchronize()
        _same(got[l], solo.serialize(), f"lane {l} vs mv_map_append")
        assert mps[l].counts.cpu().tolist() == solo.counts.cpu().tolist()
        assert np.array_equal(mps[l].poses_array(), solo.poses_array())


def test_refusal_is_per_lane(gpu, case):
    """Lane 1's match store is one row too small for the third tracked frame: that lane is refused — counts unchanged but counts[4] == 1, no row written —
    and lanes 0 and 2 are registered in full.  (The host bookkeeping that would have re-grown the store is bypassed: the kernel's own check is the subject.)"""
    from macvo_amd import _lib as L
    from macvo_amd import ops
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps

    frames, meta = _tables(all_valid_lane1=True)            # same seed: lanes 0 and 2 see the tables of `case`; lane 1 keeps all 300 rows of frames 1 and 2
    _, _, want = case
    small = 600 + 300 - 1
    maps = [DeviceVisualMap(gpu, init_size=4096), DeviceVisualMap(gpu, init_size=small), DeviceVisualMap(gpu, init_size=4096)]
    SENT_F, SENT_I = 777.0, -7
    m1 = maps[1]
    for tbl in (m1.match, m1.points):
        for k, v in tbl.items():
            v.fill_(SENT_F if v.dtype.is_floating_point else 77)
    for k in ("match2frame1", "match2frame2", "match2point", "point2match_edges", "point2match_deg"):
        m1.edges[k].fill_(SENT_I)
    for k, v in m1.frames.items():
        v[3:].fill_(1 if v.dtype == torch.bool else 55)
    for k in ("frame2match_ranges", "frame2match_num", "frame2map_ranges", "frame2map_num"):
        m1.edges[k][3:].fill_(SENT_I)
    mps = DeviceVisualMaps(maps=maps)
    lib, keep = L.load(), []
    torch.cuda.synchronize()
    for t, fr in enumerate(frames):
        if t == 3:
            torch.cuda.synchronize()
            before = m1.counts.cpu().tolist()
            assert before == [3, 600, 600, 0, 0, 0]
            snap = {k: v.clone() for tbl in (m1.frames, m1.points, m1.match, m1.edges) for k, v in tbl.items()}
        f = _lane_frame(L, fr, meta, gpu, t, t - 1, keep)
        L.check(lib.mv_map_append_lanes(C.byref(f), mps.stores_dev(), ops._stream()), "mv_map_append_lanes")
    torch.cuda.synchronize()
    assert m1.counts.cpu().tolist() == [3, 600, 600, 0, 1, 0]                    # unchanged except the error word
    for tbl in (m1.frames, m1.points, m1.match, m1.edges):
        for k, v in tbl.items():
            assert torch.equal(v, snap[k]), k                                    # nothing of the refused frame was written, inside or beyond the old size
    assert bool((m1.match["pixel1_uv"][600:] == SENT_F).all()) and bool((m1.edges["match2point"][600:] == SENT_I).all())
    assert bool((m1.frames["time_ns"][3:] == 55).all()) and bool((m1.edges["frame2match_num"][3:] == SENT_I).all())
    with pytest.raises(L.MacvoHipError, match="refused"):
        m1.sizes()
    for l in (0, 2):                                                              # the neighbours never saw it
        maps[l].n_frames = 4
        assert maps[l].counts.cpu()[4] == 0
        got = maps[l].serialize()
        ref = _oracle_lane(frames, meta, l, skip=False)
        for k, w in ref.items():
            if k != "frames//pose":                                               # (the priors here: no pose write in this test)
                assert got[k].dtype == w.dtype and np.array_equal(got[k], w, equal_nan=True), (l, k)
        assert np.array_equal(got["frames//pose"], torch.stack([fr["prior"][l] for fr in frames]).numpy())
        for k in want[l]:                                                         # ... and agree with the shared reference of the first test, row for row
            if k.startswith(("match//", "points//")):
                assert np.array_equal(got[k], want[l][k], equal_nan=True), (l, k)


# ---------------------------------------------------------------------------------------------------------------- driver
N_FRAMES, H, W = 8, 192, 256
SEEDS, SEQ_SEEDS, LOST_LANE, LOST_T = (5, 12, 33), (31, 44, 57), 1, 4
T_BS = torch.tensor([[0.05, 0.0, -0.1, 0, 0, 0, 1.0], [0.0, 0.2, 0.0, 0, 0, 0, 1.0], [-0.3, 0.1, 0.4, 0, 0, 0, 1.0]])
STARTS = torch.tensor([[3.0, -2.0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0, 0, 0, 0, 1.0], [-4.0, 2.5, 0.8, 0, 0, 0, 1.0]])


def _time(l, t):
    return 1_000_000 * (l + 1) + 33 * t


def _K(cam):
    return torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def sequences(gpu):
    from macvo_amd.pipeline import FrameInputs

    seqs = [synth.make_sequence(N_FRAMES, H, W, C=64, iters=2, seed=s) for s in SEQ_SEEDS]
    fr = seqs[LOST_LANE][1][LOST_T]                       # lane 1 only: unusable flow covariance -> no candidates -> lost track
    fr["logcov"] = fr["logcov"].clone()
    fr["logcov"][1] = 4.0
    ins = [[FrameInputs(**{k: v.to(gpu) for k, v in f.items()}, time_ns=_time(l, t)) for t, f in enumerate(s[1])] for l, s in enumerate(seqs)]
    torch.cuda.synchronize()
    return seqs[0][0], ins


def _gens(mode, seeds):
    return [int(s) for s in seeds] if mode == "device" else [torch.Generator().manual_seed(int(s)) for s in seeds]


def _want_flags(l, k):
    return [t % k != 0 or (l == LOST_LANE and t == LOST_T) for t in range(N_FRAMES)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("mode", ["device", "host"])
def test_every_lane_of_the_driver_equals_its_solo_run(gpu, sequences, mode, k):
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes
    from oracle import visual_map as VM

    cam, ins = sequences
    K = _K(cam)
    cfg = HotPathConfig(graph_type="icp", keyframe_freq=k)
    with_oracle = mode == "host" and k == 1
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=LANES, generators=_gens(mode, SEEDS), keep_extras=with_oracle)
    mps = DeviceVisualMaps(LANES, gpu, init_size=16)      # every store re-grows, at different frames in different lanes
    hot.attach_maps(mps, K, T_BS)
    batched = [stack_lanes([ins[l][t] for l in range(LANES)]) for t in range(N_FRAMES)]
    assert batched[3].lane_time_ns == [_time(l, 3) for l in range(LANES)] and batched[3].time_ns == _time(0, 3)
    hot.initialize(batched[0], init_pose=STARTS)
    assert hot.device_driven == (mode == "device")
    ora = VM.OracleVisualMap()
    meta = dict(K=K, T_BS=T_BS[0], baseline=cam["baseline"])
    ora.push_frame(meta, dict(n=0, time_ns=_time(0, 0), prior=STARTS[0]))
    prior = STARTS[0].clone()
    for t, res in enumerate(hot.run(batched[1:]), start=1):
        if with_oracle:                                   # lane 0's expected map from its own per-frame tables: the check does not rest on the one-lane path alone
            hot.sync_pose()
            torch.cuda.synchronize()
            r = res[0]
            ex, tr = r.extras, r.extras["tracked"]
            c = lambda x: x.cpu().clone()  # noqa: E731
            fr = dict(n=r.n_sel, valid=c(ex["valid"]), kp0=c(tr.kp0_uv), kp1=c(tr.kp1_uv), vals=c(tr.vals), sigma0=c(tr.sigma0), sigma1=c(tr.sigma1),
                      cov0=c(ex["cov0"]), cov1=c(ex["cov1"]), pos_Tw=c(ex["pos_Tw"]), cov0w=c(ex["cov0_w"]), color=None, time_ns=_time(0, t), prior=prior.clone())
            assert r.n_sel > 0
            idx = ora.push_frame(meta, fr)
            prior = c(r.pose)
            ora.set_pose(idx, prior)
    hot.sync_all()
    torch.cuda.synchronize()
    got = mps.serialize()
    got_poses = [m.poses_array() for m in mps]
    hot.close()
    assert any(m.cap["match"] > 16 for m in mps) and all(m.cap["frames"] >= N_FRAMES for m in mps)
    if with_oracle:
        _same(got[0], ora.serialize(), "lane 0 vs oracle")
    for l in range(LANES):
        solo = NativeHotPath(Camera(**cam), cfg, gpu, generators=_gens(mode, [SEEDS[l]]))
        sm = DeviceVisualMap(gpu, init_size=16)
        solo.attach_map(sm, K, T_BS[l])
        solo.initialize(ins[l][0], init_pose=STARTS[l])
        assert solo.device_driven == (mode == "device")
        for _ in solo.run(ins[l][1:]):
            pass
        solo.sync_all()
        torch.cuda.synchronize()
        want = sm.serialize()
        _same(got[l], want, f"lane {l} vs solo ({mode}, k={k})")
        assert np.array_equal(got_poses[l], sm.poses_array()), l
        assert mps[l].counts.cpu().tolist() == sm.counts.cpu().tolist(), l
        solo.close()
        assert got[l]["frames//need_interp"].tolist() == _want_flags(l, k), (l, got[l]["frames//need_interp"].tolist())
        assert got[l]["frames//time_ns"].tolist() == [_time(l, t) for t in range(N_FRAMES)]
        assert np.array_equal(got[l]["frames//T_BS"], T_BS[l].expand(N_FRAMES, 7).numpy())
        assert got[l]["match//pixel1_uv"].shape[0] > 100
    assert not np.array_equal(got[0]["match//pixel1_uv"][:50], got[2]["match//pixel1_uv"][:50])      # the lanes are different sequences


def test_unattached_pipes_are_unchanged_and_one_lane_forms_agree(gpu, sequences, tmp_path):
    from macvo_amd.devmap import DeviceVisualMap, DeviceVisualMaps
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    cam, ins = sequences
    K = _K(cam)
    cfg = HotPathConfig(graph_type="icp")
    two = [stack_lanes([ins[l][t] for l in range(2)]) for t in range(N_FRAMES)]

    def plain():
        hp = NativeHotPath(Camera(**cam), cfg, gpu, lanes=2, generators=[5, 12], keep_extras=True)
        hp.initialize(two[0], init_pose=STARTS[:2])
        out = []
        for res in hp.run(two[1:]):
            hp.sync_pose()
            torch.cuda.synchronize()
            # (a lane without keypoints — lane 1's lost frame — has no tables: its pose alone)
            out.append([(r.pose.clone(), r.kp0_uv.clone(), r.extras["tracked"].vals.clone(), r.extras["valid"].clone(), r.extras["cov0_w"].clone())
                        if r.n_sel else (r.pose.clone(),) for r in res])
        hp.close()
        return out

    a = plain()
    sib = NativeHotPath(Camera(**cam), cfg, gpu, lanes=2, generators=[5, 12])      # a sibling with maps, in the same process
    mps = DeviceVisualMaps(2, gpu, init_size=16)
    sib.attach_maps(mps, K)
    sib.initialize(two[0], init_pose=STARTS[:2])
    sink = torch.zeros(N_FRAMES - 1, 2, 7, device=gpu)
    for _ in sib.run(two[1:], pose_sink=sink):
        pass
    sib.sync_all()
    torch.cuda.synchronize()
    sib.close()
    b = plain()
    assert len(a) == len(b) == N_FRAMES - 1 and [len(x) for x in a[LOST_T - 1]] == [5, 1]
    for t, (fa, fb) in enumerate(zip(a, b)):
        for l in range(2):
            assert len(fa[l]) == len(fb[l])
            for x, y in zip(fa[l], fb[l]):
                assert torch.equal(x, y), (t, l)
            assert torch.equal(fa[l][0], sink[t, l]), (t, l)                      # ... and the sibling tracked the same poses, which its maps hold
    ser = mps.serialize()
    for l in range(2):
        assert np.array_equal(ser[l]["frames//pose"][1:], sink[:, l].cpu().numpy())
    mps.write([str(tmp_path / "a"), str(tmp_path / "b")])                         # MotionInterpolate + poses.npy + tensor_map.npz per lane
    assert np.load(tmp_path / "b" / "poses.npy").shape == (N_FRAMES, 8)
    assert set(np.load(tmp_path / "a" / "tensor_map.npz").files) == set(ser[0])
    # one lane: attach_map and attach_maps([m]) leave the same map
    sers = []
    for lanes_form in (False, True):
        hp = NativeHotPath(Camera(**cam), cfg, gpu, generators=[33])
        m = DeviceVisualMap(gpu, init_size=16)
        if lanes_form:
            hp.attach_maps([m], K, T_BS[2])
        else:
            hp.attach_map(m, K, T_BS[2])
        hp.initialize(ins[2][0], init_pose=STARTS[2])
        for _ in hp.run(ins[2][1:]):
            pass
        hp.sync_all()
        torch.cuda.synchronize()
        sers.append((m.serialize(), m.poses_array(), m.counts.cpu().tolist()))
        hp.close()
    _same(sers[1][0], sers[0][0], "attach_maps([m]) vs attach_map(m)")
    assert np.array_equal(sers[0][1], sers[1][1]) and sers[0][2] == sers[1][2]


def test_one_lane_c_entry_points_equal_the_lanes_path(gpu, sequences):
    """mv_frame_pipe_map_append / mv_frame_pipe_map_skip — the host-descriptor form of the one registration protocol, which Python no longer calls — made by
    hand on a pipe without maps, against the same run with ``attach_maps([m])``: lane 2's sequence, every other frame a keyframe, so both calls run."""
    from macvo_amd import _lib as L
    from macvo_amd.devmap import DeviceVisualMap
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam, ins = sequences
    seq, K, tbs, start = ins[2], _K(cam).to(gpu).contiguous(), T_BS[2].to(gpu).contiguous(), STARTS[2]
    sers = []
    for by_hand in (False, True):
        hp = NativeHotPath(Camera(**cam), HotPathConfig(graph_type="icp", keyframe_freq=2), gpu, generators=[33])
        m = DeviceVisualMap(gpu, init_size=4096)              # room for the whole run: no growth logic here
        if by_hand:                                           # frame 0 as initialize pushes it
            m.push_frame(K=K, T_BS=tbs, baseline=cam["baseline"], time_ns=_time(2, 0), prior_pose=start)
            torch.cuda.synchronize()
        else:
            hp.attach_maps([m], K, tbs)
        hp.initialize(seq[0], init_pose=start)
        lib, pipe, args = hp._lib, hp._pipe, (K.data_ptr(), tbs.data_ptr(), float(cam["baseline"]))
        for t in range(1, N_FRAMES):
            if t % 2 == 0:
                hp.step(seq[t])                               # (no finish is pending when the calls below come in)
                if by_hand:
                    L.check(lib.mv_frame_pipe_map_append(pipe, C.byref(m.stores()), m.n_frames, m.last_keyframe, *args, _time(2, t), None), "mv_frame_pipe_map_append")
                    m.last_keyframe = m.n_frames
                    m.n_frames += 1
            elif by_hand:
                L.check(lib.mv_frame_pipe_skip(pipe), "mv_frame_pipe_skip")
                L.check(lib.mv_frame_pipe_map_skip(pipe, C.byref(m.stores()), m.n_frames, *args, _time(2, t)), "mv_frame_pipe_map_skip")
                m.n_frames += 1
            else:
                hp.skip(_time(2, t))
        hp.sync_all()
        torch.cuda.synchronize()
        assert m.cap["match"] == 4096 and m.n_frames == N_FRAMES
        sers.append((m.serialize(), m.poses_array(), m.counts.cpu().tolist()))
        hp.close()
    _same(sers[1][0], sers[0][0], "mv_frame_pipe_map_append / _map_skip vs attach_maps([m])")
    assert np.array_equal(sers[0][1], sers[1][1]) and sers[0][2] == sers[1][2]
    assert sers[0][0]["frames//need_interp"].tolist() == _want_flags(2, 2) and sers[0][0]["match//pixel1_uv"].shape[0] > 100
