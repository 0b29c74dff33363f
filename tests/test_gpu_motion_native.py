"""GPU: the TartanMotionNet prior in the native frame driver (motion_model = MV_MOTION_TARTAN, ABI 7) — NativeHotPath against HotPath with the
same stand-in PoseNet (keypoints, PoseNet inputs, priors and poses bit for bit), every finish mode (host-drawn, seeded, device-driven) with
each of 2 lanes equal to its solo run, frames that lose track, the dense-mapping tail and the motion-model solve entry points."""
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Net:
    """Seeded stand-in PoseNet, lane by lane: per-plane means of [L,5,112,160] through a fixed 6x5 matrix.  Records its inputs."""

    def __init__(self, dev, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.A = (torch.randn(6, 5, generator=g) * 0.5).to(dev)
        self.b = (torch.randn(6, generator=g) * 0.3).to(dev)
        self.inputs = []

    def __call__(self, x):
        self.inputs.append(x.clone())
        # lane by lane, so that a lane of a batched pipe sees exactly the arithmetic of its solo run (a batched reduction / matmul may round differently)
        return torch.cat([torch.tanh(x[l:l + 1].clamp(-1e3, 1e3).mean(dim=(2, 3))) @ self.A.T + self.b for l in range(x.shape[0])])


def _ins(frames, dev):
    from macvo_amd.pipeline import FrameInputs

    return [FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}) for fr in frames]


@pytest.mark.parametrize("graph,min_num_point", [("disp", 10), ("icp", 10), ("disp", 100000)])
def test_native_tartan_equals_python_tartan(gpu, graph, min_num_point):
    """Host-drawn frames on torch's global generator: the driver's PoseNet input (MV_FB_MOTION_IN), prior (MV_FB_PRIOR), keypoints and poses are
    HotPath's bits.  min_num_point = 100000: every frame loses track inside the solve and keeps its prior, and the next prior composes onto it."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    n_frames = 6
    cam, frames, _ = synth.make_sequence(n_frames, 240, 320, C=64, iters=3, seed=21)
    ins = _ins(frames, gpu)
    cfg = HotPathConfig(graph_type=graph, motion_model="tartan", min_num_point=min_num_point)
    na, nb = _Net(gpu), _Net(gpu)
    py = HotPath(Camera(**cam), cfg, gpu, pose_net=na)
    nat = NativeHotPath(Camera(**cam), cfg, gpu, pose_net=nb)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    prev = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)
    for t in range(1, n_frames):
        torch.manual_seed(300 + t)
        a = py.step(ins[t])
        torch.manual_seed(300 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(_bits(na.inputs[-1]), _bits(nb.inputs[-1])), t
        assert torch.equal(a.kp0_uv, b.kp0_uv), t
        assert torch.equal(_bits(a.prior), _bits(b.prior)), t
        want = ops.pose_exp_compose(prev, nb(nb.inputs[-1]).reshape(6))
        nb.inputs.pop()
        assert torch.equal(_bits(b.prior), _bits(want)), t
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info), t
        assert torch.equal(_bits(a.pose), _bits(b.pose)), t
        if min_num_point > 1000:
            assert torch.equal(_bits(b.pose), _bits(b.prior)) and int(b.info[0, 1].item()) == 0, t
        prev = b.pose.clone()
    assert (prev - torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)).abs().max() > 1e-3
    nat.close()


def _lane_frames(lanes, n_frames, seed0):
    seqs = [synth.make_sequence(n_frames, 192, 256, C=64, iters=2, seed=seed0 + 13 * l) for l in range(lanes)]
    return seqs[0][0], [s[1] for s in seqs]


@pytest.mark.parametrize("mode", ["host", "seeded", "device"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_native_tartan_finish_modes_and_lanes_equal_solo_runs(gpu, monkeypatch, mode, lanes):
    """Every finish mode of the driver with the prior: host-drawn (mv_frame_pipe_finish, torch generators), seeded (mv_frame_pipe_finish_seeded) and
    device-driven (mv_frame_pipe_finish_device), through run(): each lane's priors and poses equal its solo run's bits."""
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    monkeypatch.setenv("MV_PIPE_DEVICE_DRAW", "0" if mode == "seeded" else "1")
    n_frames = 5
    cam, per_lane = _lane_frames(lanes, n_frames, 31)
    ins = [_ins(fr, gpu) for fr in per_lane]
    seeds = [5 + 7 * l for l in range(lanes)]
    gens = (lambda: [torch.Generator().manual_seed(s) for s in seeds]) if mode == "host" else (lambda: list(seeds))
    cfg = HotPathConfig(graph_type="icp", motion_model="tartan")
    hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=gens(), pose_net=_Net(gpu))
    stacked = [stack_lanes([ins[l][t] for l in range(lanes)]) for t in range(n_frames)]
    hot.initialize(stacked[0])
    assert hot.device_driven == (mode == "device")
    poses, priors = [], []
    for res in hot.run(stacked[1:]):
        rs = res if isinstance(res, list) else [res]
        hot.sync_pose()       # (run() hands results out before their solves finish: the views are read behind them)
        poses.append(torch.stack([r.pose.clone() for r in rs]))
        priors.append(torch.stack([r.prior.clone() for r in rs]))
    torch.cuda.synchronize()
    hot.close()
    for l in range(lanes):
        solo = NativeHotPath(Camera(**cam), cfg, gpu, lanes=1, generators=[gens()[l]], pose_net=_Net(gpu))
        solo.initialize(ins[l][0])
        for t, res in enumerate(solo.run(ins[l][1:])):
            solo.sync_pose()
            torch.cuda.synchronize()
            assert torch.equal(_bits(res.prior), _bits(priors[t][l])), (mode, lanes, l, t)
            assert torch.equal(_bits(res.pose), _bits(poses[t][l])), (mode, lanes, l, t)
        solo.close()
    assert (priors[-1] - poses[-2]).abs().max() > 1e-4      # the prior moved off the previous pose


def test_native_tartan_without_candidates_keeps_the_prior(gpu):
    """No candidates at all (the driver's n_max == 0 branch): the frame's pose is its composed prior, and the next prior composes onto it."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam, frames, _ = synth.make_sequence(4, 240, 320, C=64, iters=1, seed=4)
    ins = _ins(frames, gpu)
    net = _Net(gpu, seed=3)
    nat = NativeHotPath(Camera(**cam), HotPathConfig(max_match_cov=0.0, motion_model="tartan"), gpu, pose_net=net)
    nat.initialize(ins[0])
    prev = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)
    for t in range(1, 4):
        r = nat.step(ins[t])
        torch.cuda.synchronize()
        assert r.n_sel == 0
        want = ops.pose_exp_compose(prev, net(net.inputs[-1]).reshape(6))
        assert torch.equal(_bits(r.pose), _bits(want)) and torch.equal(_bits(r.prior), _bits(want)), t
        prev = r.pose.clone()
    nat.close()


def test_native_tartan_mapping_tail_registers_with_the_previous_pose(gpu):
    """mapping = True with the prior: the dense map points are registered with the previous frame's pose (prev_pose.Act, MACVO.py:334), not the prior —
    the driver's MV_FB_MAP_* tables equal HotPath's map points bit for bit, and their world positions follow the previous pose."""
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath
    from oracle import se3

    H, W, n_frames = 240, 320, 4
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=1, seed=23)
    cfg = HotPathConfig(mapping=True, map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=500, graph_type="icp", motion_model="tartan")
    py = HotPath(Camera(**cam), cfg, gpu, pose_net=_Net(gpu))
    nat = NativeHotPath(Camera(**cam), cfg, gpu, pose_net=_Net(gpu))
    ins = _ins(frames, gpu)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    seen = 0
    prev = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    for t in range(1, n_frames):
        torch.manual_seed(70 + t)
        a = py.step(ins[t])
        torch.manual_seed(70 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.prior), _bits(b.prior)) and torch.equal(_bits(a.pose), _bits(b.pose)), t
        ma, mb = a.map_points, b.map_points
        assert (ma is None) == (mb is None), t
        if mb is not None:
            assert torch.equal(ma.uv, mb.uv) and torch.equal(_bits(ma.pos_Tw), _bits(mb.pos_Tw)), t
            want = se3.se3_act(prev, mb.pos_Tc.cpu())
            assert (mb.pos_Tw.cpu() - want).abs().max() <= 1e-4, t
            off = se3.se3_act(b.prior.cpu(), mb.pos_Tc.cpu())
            assert (mb.pos_Tw.cpu() - off).abs().max() > 1e-4, t     # (the prior would have registered them elsewhere)
            seen += mb.uv.shape[0]
        prev = b.pose.cpu().clone()
    assert seen > 0
    nat.close()


def test_static_pipe_has_no_motion_views_and_tartan_needs_a_net(gpu):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath

    cam, frames, _ = synth.make_sequence(2, 240, 320, C=64, iters=1, seed=4)
    ins = _ins(frames, gpu)
    st = NativeHotPath(Camera(**cam), HotPathConfig(), gpu)
    st.initialize(ins[0])
    r = st.step(ins[1])
    assert r.prior is None
    with pytest.raises(ops.L.MacvoHipError):
        st._view("MOTION_IN", 0, torch.float32, (1, 5, 112, 160))
    with pytest.raises(ops.L.MacvoHipError):
        ops.L.check(st._lib.mv_frame_pipe_set_motion(st._pipe, r.pose.data_ptr(), ops._stream()), "mv_frame_pipe_set_motion")
    st.close()
    mo = NativeHotPath(Camera(**cam), HotPathConfig(motion_model="tartan"), gpu)
    mo.initialize(ins[0])
    with pytest.raises(ops.L.MacvoHipError):
        mo.step(ins[1])
    mo.close()
