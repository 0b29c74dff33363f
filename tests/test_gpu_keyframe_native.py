"""GPU: the local-frame solve and the keyframe policy in the plugin, ``HotPath`` and the native frame driver.

* ``HotPath`` (``solve_frame``, ``keyframe_freq``, ``skip``) with a ``DeviceVisualMap`` against the reference's own loop (tests/golden/keyframe_run.npz:
  AllKeyframe / UniformKeyframe 2 and 3 x TwoFrame_PGO / Local_TwoFrame_PGO) under the bars of test_gpu_covfree.py: stored rows and keypoints bit for
  bit, covariances 5e-5, poses 1e-4 — the skipped frames' through ``DeviceVisualMap.motion_interpolate`` — and the flags as pushed (index % k != 0);
* ``HIP_Local_TwoFrame_PGO`` in ``run_pair``'s call order (write_map, push, start_optimize(get_graph_data)) on the golden's stored rows: with k = 3
  ``pose[frame_idx - 1]`` is a skipped row holding a stale prior, and the golden's poses only come out if that row is what the solve uses;
* ``NativeHotPath`` with an attached map equals ``HotPath`` bit for bit — keypoints, poses, the whole serialised map — for k in {1, 2, 3} x {world,
  local} in every finish mode (host-drawn, seeded, device-driven, explicit keypoints), with ``motion_model="tartan"`` on a stand-in PoseNet, and at 2
  lanes for ``solve_frame`` alone;
* a run started about 1350 m from the origin (each component below 1024 m: see the test): every local solve equals the torch restatement (tests/local_pgo_ref.py around ``oracle.pgo.solve``) on
  the frame's own tables to 1e-4, and the world-frame run of the same frames does not — the test can tell the two apart.

Reads only committed .npz data, never the reference tree."""
from dataclasses import replace
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import keyframe_golden as KG
from tests import local_pgo_ref as LR
from tests import refrun, synth
from tests.test_gpu_covfree import POSE_TOL, _inputs, check_frame_against_golden
from tests.test_gpu_motion_native import _Net

pytestmark = pytest.mark.gpu
FILTERS = {"compose": 7, "sanity": 1}
IDENT = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cfg_of(spec, **kw):
    from macvo_amd.pipeline import HotPathConfig

    base, _, (kf, freq), opt, graph = spec
    c = refrun.CASES[base]
    return HotPathConfig(selector="nodepth" if c["selector"].endswith("NoDepth") else "full", graph_type=graph, filters=FILTERS[c["outlier"]],
                         mapping=c["mapping"], solve_frame="local" if opt.startswith("Local") else "world", keyframe_freq=freq or 1, **kw)


def _K(cam):
    return torch.tensor([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])


def _push_keyframe(dmap, cam, K, time_ns, prior, r):
    """A HotPath keyframe into the device map, as MACVO.run_pair registers it (the driver-less path: the caller owns the map)."""
    ex = r.extras
    idx = dmap.push_frame(K=K, T_BS=IDENT, baseline=cam["baseline"], time_ns=time_ns, prior_pose=prior, tracked=ex["tracked"], valid=ex["valid"],
                          cov0=ex["cov0"], cov1=ex["cov1"], pos_Tw=ex["pos_Tw"], cov0_world=ex["cov0_w"])
    dmap.set_pose(idx, r.pose)
    return idx


@pytest.mark.parametrize("name", sorted(KG.meta()["cases"]))
def test_hot_path_with_keyframes_matches_the_reference_loop(gpu, name):
    from macvo_amd.devmap import DeviceVisualMap
    from macvo_amd.pipeline import Camera, HotPath

    meta = KG.meta()
    spec = meta["cases"][name]
    k = spec[2][1] or 1
    g = KG.case(name)
    cam, maps, _ = refrun.tartanair_maps()
    maps = maps * spec[1]
    ins = [replace(x, time_ns=1_000_000 * (t + 1)) for t, x in enumerate(_inputs(maps, cam, gpu, True, True, sigma2=True))]
    K = _K(cam)
    torch.manual_seed(meta["seed"])                      # the selectors consume the global CPU generator, as the reference's do
    hot = HotPath(Camera(**cam), _cfg_of(spec), gpu, keep_extras=True)
    dmap = DeviceVisualMap(gpu, init_size=64)
    hot.attach_map(dmap, K)
    hot.initialize(ins[0])
    dmap.push_frame(K=K, T_BS=IDENT, baseline=cam["baseline"], time_ns=ins[0].time_ns, prior_pose=IDENT)
    prior = IDENT.to(gpu)
    # the keyframes' poses as solved: the serialised ones where nothing is interpolated; with skipped frames MotionInterpolate rebuilds every pose behind
    # the first interpolated motion, so there it is the snapshot taken before terminate — whose last keyframe still sits at its prior (its result is
    # written by terminate): that one row is pinned by the comparison after motion_interpolate below only
    last_key = (len(ins) - 1) // k * k
    solved = dict(g)
    if k > 1:
        solved["map/frames//pose"] = g["pose_before_terminate"].copy()
    for t in range(1, len(ins)):
        if t % k:
            hot.skip(ins[t].time_ns)
            continue
        r = hot.step(ins[t])
        torch.cuda.synchronize()
        if k > 1 and t == last_key:
            solved["map/frames//pose"][t] = r.pose.cpu().numpy()
        check_frame_against_golden(solved, t, r.extras, r.kp0_uv, r.pose, True, True, f"HotPath {name}", exact_variances=True)
        assert _push_keyframe(dmap, cam, K, ins[t].time_ns, prior, r) == t
        prior = r.pose.clone()
    torch.cuda.synchronize()
    n = len(ins)
    ser = dmap.serialize()
    assert np.array_equal(ser["frames//need_interp"], g["need_interp_pushed"]) and np.array_equal(ser["frames//need_interp"], np.arange(n) % k != 0)
    assert np.array_equal(ser["edge/frame2match/ranges"], g["map/edge/frame2match/ranges"])                 # a skipped row has none, keyframes chain over them
    assert np.array_equal(ser["frames//time_ns"], 1_000_000 * (np.arange(n) + 1)) and int(dmap.counts.cpu()[3]) == 0
    before = g["pose_before_terminate"]
    for t in range(1, n):
        if t % k:                                        # the pose the previous keyframe was pushed with, not its optimised pose
            dp = np.abs(ser["frames//pose"][t] - before[t]).max()
            assert dp <= POSE_TOL, (name, t, dp)
            assert np.array_equal(ser["frames//pose"][t], ser["frames//pose"][t - 1] if (t - 1) % k else (ser["frames//pose"][t - 1 - k] if t - 1 >= k else IDENT.numpy()))
    n_interp = dmap.motion_interpolate()
    assert n_interp == int(g["map/frames//need_interp"].sum()) and (k == 1 or n_interp >= 1)
    torch.cuda.synchronize()
    dp = np.abs(dmap.frames["pose"][:n].cpu().numpy() - g["map/frames//pose"]).max()
    dn = np.abs(dmap.poses_array()[:, 1:] - g["poses_npy"][:, 1:]).max()
    print(f"HotPath {name}: {n_interp} interpolated motions, max pose difference after MotionInterpolate {dp:.3e}, poses.npy {dn:.3e} (bound {POSE_TOL})")
    assert dp <= POSE_TOL and dn <= POSE_TOL, (name, dp, dn)


# ------------------------------------------------------------------------------------------------------------------ plugin
class _Bundle:
    def __init__(self, data):
        self.data = data


class _MirrorMap:
    """What (HIP_)Local_TwoFrame_PGO touches of a VisualMap: ``frames.data["pose"]``, ``frames[idx]``, ``get_frame2match``, ``get_match2point``."""

    def __init__(self, n, K, baseline):
        pose = IDENT.repeat(n, 1).clone()
        outer = self

        class Frames:
            data = {"pose": pose}

            def __getitem__(self, idx):
                i = int(idx)
                return _Bundle({"K": K[None], "pose": pose[i: i + 1], "baseline": torch.tensor([baseline]), "index": i})

        self.frames = Frames()
        self.rows = {}

    def get_frame2match(self, frame):
        return _Bundle(self.rows[frame.data["index"]][0])

    def get_match2point(self, obs):
        return _Bundle(next(p for o, p in self.rows.values() if o is obs.data))


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("name", ["u3_local_icp", "u2_local_icp", "u3_local_disp", "all_local_reproj"])
def test_local_plugin_in_run_pair_order(gpu, name, parallel):
    from macvo_amd.plugins import HIP_Local_TwoFrame_PGO

    spec = KG.meta()["cases"][name]
    k = spec[2][1] or 1
    g = KG.case(name)
    cam, _, _ = refrun.tartanair_maps()
    n = g["need_interp_pushed"].shape[0]
    cfg = NS(device="cuda", vectorize=True, parallel=parallel, graph_type=spec[4], autodiff=False)
    HIP_Local_TwoFrame_PGO.is_valid_config(cfg)
    opt = HIP_Local_TwoFrame_PGO(cfg)
    vmap = _MirrorMap(n, _K(cam), cam["baseline"])
    pose = vmap.frames.data["pose"]
    ranges = g["map/edge/frame2match/ranges"]
    prev_key = 0
    for t in range(1, n):
        if t % k:                                                           # MACVO.py:177-179: before write_map, so the row holds the keyframe's prior
            pose[t] = pose[prev_key]
            continue
        opt.write_map(vmap)                                                 # :187
        lo, cnt = int(ranges[t, 0, 0]), int(ranges[t, 0, 1])
        tt = lambda key: torch.from_numpy(g[key][lo:lo + cnt])  # noqa: E731
        obs = {f: tt(f"map/match//{f}") for f in ("pixel2_uv", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_uv_cov", "obs2_covTc")}
        vmap.rows[t] = (obs, {"pos_Tw": tt("map/points//pos_Tw"), "cov_Tw": tt("map/points//cov_Tw")})
        pose[t] = pose[prev_key]                                            # push_keyframe(frame1, est_pose): StaticMotionModel (:193-194,282)
        prev_key = t
        gin = opt.get_graph_data(vmap, torch.tensor([t]))
        assert torch.equal(gin.ref_pose.reshape(7), pose[t - 1]) and int(opt.T_o2w_idx) == t - 1
        opt.start_optimize(gin)                                             # :309-311
    opt.write_map(vmap)                                                     # terminate (:373-376)
    opt.terminate()
    # The golden's snapshot before terminate: every keyframe but the last at its optimised pose (written back by the next run_pair), the skipped rows at
    # the prior they were pushed with.  The last keyframe's result is written by terminate: serialised as it is where nothing is interpolated (k = 1);
    # with skipped frames MotionInterpolate then rebuilds it, and the HotPath test above holds it through motion_interpolate.
    before, after = g["pose_before_terminate"], g["map/frames//pose"]
    worst = 0.0
    for t in range(1, n):
        if t != prev_key:
            worst = max(worst, float(np.abs(pose[t].numpy() - before[t]).max()))
        elif k == 1:
            worst = max(worst, float(np.abs(pose[t].numpy() - after[t]).max()))
    print(f"HIP_Local_TwoFrame_PGO {name} parallel={parallel}: max pose difference {worst:.3e} (bound {POSE_TOL})")
    assert worst <= POSE_TOL, (name, worst)
    assert pose.dtype == torch.float32 and (pose[prev_key] - pose[prev_key - k]).abs().max() > 1e-3


def test_local_plugin_rereads_its_reference_row(gpu):
    """write_graph_data re-reads pose[T_o2w_idx] (Optimizer.py:128-129): with the row as it was, the kernel's fp32 world pose is written; had the row
    changed, the local-frame result is re-expressed with its new pose — NormalizeQuat(T_o2w @ T_c2o) — as the reference would."""
    import json
    import os

    from macvo_amd.plugins import HIP_Local_TwoFrame_PGO
    from tests.test_local_keyframe_host import GOLD, problem, stage

    z = np.load(GOLD)
    gold = {key: z[key] for key in z.files}
    gold["meta"] = json.loads(str(gold["meta"]))
    prob, ref = problem(gold, 2)                                            # the case with ref_pose != init_pose
    vmap = _MirrorMap(2, prob.K, prob.baseline)
    pose = vmap.frames.data["pose"]
    pose[0], pose[1] = ref, prob.init_pose
    vmap.rows[1] = ({f: getattr(prob, f) for f in ("pixel2_uv", "pixel2_d", "pixel2_disp", "pixel2_disp_cov", "pixel2_uv_cov", "obs2_covTc")},
                    {"pos_Tw": prob.pos_Tw, "cov_Tw": prob.cov_Tw})
    for moved in (False, True):
        pose[0], pose[1] = ref, prob.init_pose
        opt = HIP_Local_TwoFrame_PGO(NS(device="cuda", vectorize=True, parallel=False, graph_type="icp", autodiff=False))
        opt.start_optimize(opt.get_graph_data(vmap, torch.tensor([1])))
        res = opt.get_result()
        assert res.motion.dtype == torch.float64 and float((res.motion[0] - stage(gold, 2, "icp", "pose_local")).abs().max()) <= 1e-8
        if moved:
            pose[0] = LR.normalize_quat(ref + torch.tensor([0.5, 0, 0, 0, 0, 0, 0]))
        opt.write_map(vmap)
        # (row unchanged: the kernel's own world pose = the golden's bits.  Row moved: the plugin's host-side torch form against the restatement's — the same
        # torch ops on the same host, fused cross product or not)
        want = stage(gold, 2, "icp", "pose_world_f32") if not moved else LR.optim_to_world(res.motion[0], pose[0])
        assert torch.equal(pose[1], want), (moved, pose[1], want)


# ------------------------------------------------------------------------------------------------------------------ native driver
def _synth_inputs(gpu, n_frames, seed=8, H=240, W=320):
    from macvo_amd.pipeline import FrameInputs

    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=32, iters=2, seed=seed)
    ins = [FrameInputs(**{key: v.to(gpu) for key, v in fr.items()}, time_ns=1000 + 33 * t) for t, fr in enumerate(frames)]
    torch.cuda.synchronize()
    return cam, ins


def _explicit_rows(n_frames, cam, num=150):
    g = torch.Generator().manual_seed(77)
    return [torch.stack([torch.randint(40, cam["W"] - 40, (num,), generator=g), torch.randint(40, cam["H"] - 40, (num,), generator=g)], dim=1) for _ in range(n_frames)]


@pytest.mark.parametrize("mode", ["host", "seeded", "device", "explicit"])
@pytest.mark.parametrize("frame", ["world", "local"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_native_driver_with_map_equals_hot_path(gpu, monkeypatch, k, frame, mode):
    from macvo_amd.devmap import DeviceVisualMap
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
    n_frames = 11
    cam, ins = _synth_inputs(gpu, n_frames)
    if mode == "explicit":
        ins = [replace(x, keypoints=kp) for x, kp in zip(ins, _explicit_rows(n_frames, cam))]
    K = _K(cam)
    T_BS = torch.tensor([0.05, 0.0, -0.1, 0.0, 0.0, 0.0, 1.0])
    start = torch.tensor([3.0, -2.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    cfg = HotPathConfig(graph_type="icp", solve_frame=frame, keyframe_freq=k, selector="explicit" if mode == "explicit" else "nodepth")
    seed = 41
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True, generator=torch.Generator().manual_seed(seed))
    nat = NativeHotPath(Camera(**cam), cfg, gpu, generators=[torch.Generator().manual_seed(seed)] if mode in ("host", "explicit") else [seed])
    ma, mb = DeviceVisualMap(gpu, init_size=64), DeviceVisualMap(gpu, init_size=64)
    py.attach_map(ma, K, T_BS)
    nat.attach_map(mb, K, T_BS)
    py.initialize(ins[0], init_pose=start)
    nat.initialize(ins[0], init_pose=start)
    assert nat.device_driven == (mode == "device")
    ma.push_frame(K=K, T_BS=T_BS, baseline=cam["baseline"], time_ns=ins[0].time_ns, prior_pose=start)
    keys = [t for t in range(1, n_frames) if t % k == 0]
    prior, res_a = start.to(gpu), []
    for i, r in enumerate(py.run(ins[1:])):              # (run to its end: the frames behind the last keyframe are skipped there)
        t = keys[i]
        py.sync_pose()
        torch.cuda.synchronize()
        ex = r.extras
        idx = ma.push_frame(K=K, T_BS=T_BS, baseline=cam["baseline"], time_ns=ins[t].time_ns, prior_pose=prior, tracked=ex["tracked"], valid=ex["valid"],
                            cov0=ex["cov0"], cov1=ex["cov1"], pos_Tw=ex["pos_Tw"], cov0_world=ex["cov0_w"])
        assert idx == t
        ma.set_pose(idx, r.pose)
        prior = r.pose.clone()
        res_a.append((r.kp0_uv.clone(), r.pose.clone()))
    res_b = []
    for r in nat.run(ins[1:]):
        nat.sync_pose()
        res_b.append((r.kp0_uv.clone(), r.pose.clone()))
    torch.cuda.synchronize()
    nat.sync_all()
    torch.cuda.synchronize()
    assert len(res_a) == len(res_b) == len(keys)
    for t, (a, b) in zip(keys, zip(res_a, res_b)):
        assert torch.equal(a[0], b[0]), (t, "keypoints")
        assert torch.equal(_bits(a[1]), _bits(b[1])), (t, "pose", a[1], b[1])
    sa, sb = ma.serialize(), mb.serialize()
    assert set(sa) == set(sb)
    for key, w in sa.items():
        assert sb[key].dtype == w.dtype and np.array_equal(sb[key], w, equal_nan=True), key
    assert np.array_equal(sb["frames//need_interp"], np.arange(n_frames) % k != 0) and ma.counts.cpu().tolist() == mb.counts.cpu().tolist()
    assert sb["frames//time_ns"].tolist() == [1000 + 33 * t for t in range(n_frames)]
    assert ma.motion_interpolate() == mb.motion_interpolate()
    assert torch.equal(_bits(ma.frames["pose"][:n_frames]), _bits(mb.frames["pose"][:n_frames]))
    nat.close()


@pytest.mark.parametrize("mode", ["host", "seeded", "device"])
@pytest.mark.parametrize("frame", ["world", "local"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_native_driver_with_the_motion_model_equals_hot_path(gpu, monkeypatch, k, frame, mode):
    """motion_model "tartan" on a stand-in PoseNet: the prior a skipped row carries and a local solve behind it refers to is MV_FB_PRIOR.  Host-drawn
    frames on torch's global generator, seeded and device-driven ones on the driver's own generator against HotPath on the same seed."""
    from macvo_amd.devmap import DeviceVisualMap
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    n_frames = 8
    cam, ins = _synth_inputs(gpu, n_frames, seed=21)
    K = _K(cam)
    monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
    cfg = HotPathConfig(graph_type="icp", solve_frame=frame, keyframe_freq=k, motion_model="tartan")
    own = mode != "host"
    py = HotPath(Camera(**cam), cfg, gpu, keep_extras=True, pose_net=_Net(gpu), generator=torch.Generator().manual_seed(23) if own else None)
    nat = NativeHotPath(Camera(**cam), cfg, gpu, pose_net=_Net(gpu), generators=[23] if own else None)
    ma, mb = DeviceVisualMap(gpu, init_size=64), DeviceVisualMap(gpu, init_size=64)
    py.attach_map(ma, K)
    nat.attach_map(mb, K)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    assert nat.device_driven == (mode == "device")
    ma.push_frame(K=K, T_BS=IDENT, baseline=cam["baseline"], time_ns=ins[0].time_ns, prior_pose=None)
    moved = 0.0
    for t in range(1, n_frames):
        if t % k:
            py.skip(ins[t].time_ns)
            nat.skip(ins[t].time_ns)
            continue
        torch.manual_seed(300 + t)
        a = py.step(ins[t])
        torch.manual_seed(300 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(a.kp0_uv, b.kp0_uv) and torch.equal(_bits(a.prior), _bits(b.prior)) and torch.equal(_bits(a.pose), _bits(b.pose)), t
        moved = max(moved, float((a.prior - a.pose).abs().max()))
        _push_keyframe(ma, cam, K, ins[t].time_ns, a.prior, a)
    torch.cuda.synchronize()
    sa, sb = ma.serialize(), mb.serialize()
    for key, w in sa.items():
        assert np.array_equal(sb[key], w, equal_nan=True), key
    assert moved > 1e-4 and np.array_equal(sb["frames//need_interp"], np.arange(n_frames) % k != 0)
    nat.close()


def test_native_driver_two_lanes_local_equal_solo_runs(gpu):
    """``solve_frame`` works for any lane count (keyframes with a map are one lane per pipe, as the map is)."""
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath, stack_lanes

    n_frames, lanes = 5, 2
    seqs = [synth.make_sequence(n_frames, 192, 256, C=64, iters=2, seed=31 + 13 * l) for l in range(lanes)]
    cam = seqs[0][0]
    ins = [[FrameInputs(**{key: v.to(gpu) for key, v in fr.items()}) for fr in s[1]] for s in seqs]
    starts = torch.tensor([[3.0, -2.0, 1.0, 0, 0, 0, 1.0], [-40.0, 25.0, 8.0, 0, 0, 0, 1.0]])
    cfg = HotPathConfig(graph_type="icp", solve_frame="local")
    seeds = [5, 12]
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=list(seeds))
    hot.initialize(stack_lanes([ins[l][0] for l in range(lanes)]), init_pose=starts)
    poses = []
    for res in hot.run([stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(1, n_frames)]):
        hot.sync_pose()
        poses.append(torch.stack([r.pose.clone() for r in res]))
    torch.cuda.synchronize()
    hot.close()
    for l in range(lanes):
        for fr, differs in (("local", False), ("world", True)):
            solo = NativeHotPath(Camera(**cam), replace(cfg, solve_frame=fr), gpu, generators=[seeds[l]])
            solo.initialize(ins[l][0], init_pose=starts[l])
            same = True
            for t, res in enumerate(solo.run(ins[l][1:])):
                solo.sync_pose()
                torch.cuda.synchronize()
                same = same and torch.equal(_bits(res.pose), _bits(poses[t][l]))
            solo.close()
            assert same != differs, (l, fr)


# ------------------------------------------------------------------------------------------------------------------ far from the origin
def _problem_of(r, cam, init_pose):
    """The frame's own solve as an oracle problem: the rows the observation filters kept."""
    from oracle import pgo

    ex = r.extras
    tr, v = ex["tracked"], ex["valid"].bool().cpu()
    c = lambda t: t.cpu()[v]  # noqa: E731
    vals = tr.vals.cpu()
    return pgo.PGOProblem(init_pose=init_pose.cpu().float(), K=_K(cam), baseline=cam["baseline"], pos_Tw=c(ex["pos_Tw"]), cov_Tw=c(ex["cov0_w"]),
                          pixel2_uv=c(tr.kp1_uv), pixel2_d=vals[4][v][:, None], pixel2_disp=vals[5][v][:, None], pixel2_disp_cov=vals[6][v][:, None],
                          pixel2_uv_cov=c(tr.sigma1), obs2_covTc=c(ex["cov1"]))


@pytest.mark.parametrize("graph", ["icp", "disp"])
def test_far_from_the_origin_local_is_the_restatement_and_world_is_not(gpu, graph):
    """initialize(init_pose) about 1350 m out (every component below 1024 m, so one fp32 ulp of a pose component, 6.1e-5, stays below the 1e-4 bar):
    each local solve of the run equals ``local_pgo_ref.solve`` on the frame's own tables and reference pose to 1e-4; the world-frame run of the same
    frames — same keypoints, same start — leaves that trajectory by more than the bar."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig
    from oracle import se3

    n_frames = 7
    cam, ins = _synth_inputs(gpu, n_frames, seed=14)
    q = se3.so3_exp(torch.tensor([0.5, -0.7, 0.6], dtype=torch.float64)).float()
    start = torch.cat([torch.tensor([900.0, -800.0, 600.0]), q])
    runs = {}
    for frame in ("local", "world"):
        hot = HotPath(Camera(**cam), HotPathConfig(graph_type=graph, solve_frame=frame), gpu, keep_extras=True, generator=torch.Generator().manual_seed(9))
        hot.initialize(ins[0], init_pose=start)
        prev, out = start.clone(), []
        for t in range(1, n_frames):
            r = hot.step(ins[t])
            torch.cuda.synchronize()
            want = LR.solve(_problem_of(r, cam, prev), prev, graph, min_points=10).pose_f32
            out.append((r.pose.cpu().clone(), want))
            prev = r.pose.cpu().clone()
        runs[frame] = out
    worst_local = max(float((got - want).abs().max()) for got, want in runs["local"])
    # the oracle trajectory is the local run's restatement; the world run saw the same frames and keypoints
    worst_world = max(float((w[0] - l[1]).abs().max()) for w, l in zip(runs["world"], runs["local"]))
    print(f"far origin, {graph}: local run vs restatement {worst_local:.3e}, world run vs restatement {worst_world:.3e} (bound {POSE_TOL})")
    assert worst_local <= POSE_TOL, worst_local
    assert worst_world > POSE_TOL, worst_world
