"""GPU: the TartanMotionNet motion prior — mv_motion_input_lanes bitwise against the torch restatement (tests/motion_model_ref.py)
run by torch on the device, mv_pose_exp_compose against the PyPose shim, and HotPath with a stand-in pose net: a zero-motion net is
the static pipe bit for bit, a lost-track frame keeps the composed prior, and a sequence equals the oracle's loop with the prior
substituted."""
import pytest
import torch

from tests import motion_model_ref as R
from tests.golden import pypose_shim as pp

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _maps(H, W, lanes, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    flow = torch.randn(lanes, 2, H, W, generator=g) * 8
    depth = 0.5 + 20 * torch.rand(lanes, 1, H, W, generator=g)
    if special:
        # NaN, 0, negative and +-inf depths, scattered and in blocks that the bilinear taps straddle
        n = H * W
        flat = depth.view(lanes, -1)
        idx = torch.randperm(n, generator=g)[: n // 50]
        q = idx.numel() // 5
        flat[:, idx[:q]] = float("nan")
        flat[:, idx[q:2 * q]] = 0.0
        flat[:, idx[2 * q:3 * q]] = -3.0
        flat[:, idx[3 * q:4 * q]] = float("inf")
        flat[:, idx[4 * q:]] = -float("inf")
        depth[:, :, H // 2: H // 2 + 9, W // 3: W // 3 + 13] = 0.0
        depth[:, :, H // 3: H // 3 + 7, W // 2: W // 2 + 5] = float("nan")
    return flow, depth


CAM = dict(fx=320.0, fy=321.5, cx=319.5, cy=239.25, baseline=0.25)


@pytest.mark.parametrize("H,W,lanes,special", [(480, 640, 1, False), (480, 640, 4, True), (720, 1280, 1, True), (720, 1280, 4, False),
                                               (485, 651, 1, True), (485, 651, 4, True), (112, 160, 1, True), (113, 161, 2, True),
                                               (300, 700, 1, True)])
def test_motion_input_bitwise_against_torch_on_device(gpu, H, W, lanes, special):
    from macvo_amd import ops

    flow, depth = _maps(H, W, lanes, 11 + H + lanes, special)
    flow, depth = flow.to(gpu), depth.to(gpu)
    out = ops.motion_input(flow, depth, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["baseline"])
    assert out.shape == (lanes, 5, 112, 160)
    for lane in range(lanes):
        ref = R.motion_input(flow[lane: lane + 1], depth[lane: lane + 1], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["baseline"])
        for c in range(5):
            a, b = out[lane, c], ref[0, c]
            same = (_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))
            assert bool(same.all()), (lane, c, int((~same).sum()), (a - b).abs().nan_to_num().max().item())
    if special:   # the special depths reached the depth channel: zeros from NaN / negative / inf, FLT_MAX-derived values from 0
        dch = out[:, 2]
        assert bool((dch == 0).any()) and not bool(torch.isnan(dch).any())


def test_motion_input_lane_layout(gpu):
    """[L,2,H,W] / [L,1,H,W] lanes = each lane alone; [2,H,W] + [H,W] = one lane."""
    from macvo_amd import ops

    flow, depth = _maps(480, 640, 3, 5, True)
    flow, depth = flow.to(gpu), depth.to(gpu)
    out = ops.motion_input(flow, depth, *[CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    for lane in range(3):
        one = ops.motion_input(flow[lane], depth[lane, 0], *[CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
        assert torch.equal(_bits(one[0]), _bits(out[lane]))


def _poses(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, 3, generator=g, dtype=torch.float64) * 3
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    return torch.cat([t, q], 1)


def test_pose_exp_compose_against_shim(gpu):
    from macvo_amd import ops

    n = 96
    prev = _poses(n, 3)
    g = torch.Generator().manual_seed(4)
    raw = torch.randn(n, 6, generator=g, dtype=torch.float64)
    raw[:32] *= 1e-6        # small angles: |phi| ~ 1e-8 < fp32 eps -> the Taylor branch
    raw[32:64] *= 30        # large angles: |phi| ~ 0.4 .. 1 rad
    raw[64:70] = 0.0        # zero motion
    prev32, raw32 = prev.float(), raw.float()
    out = ops.pose_exp_compose(prev32.to(gpu), raw32.to(gpu)).cpu()
    ref64 = R.compose(prev32.double(), raw32.double(), pp)
    ref32 = R.compose(prev32, raw32, pp)
    # fp32 arithmetic over |t| ~ 10: a few ulps of the translation, the quaternion at fp32 roundoff
    assert (out.double() - ref64).abs()[:, :3].max() <= 64 * 2.0 ** -23 * 10
    assert (out.double() - ref64).abs()[:, 3:].max() <= 16 * 2.0 ** -23
    assert (out - ref32).abs()[:, 3:].max() <= 16 * 2.0 ** -23
    # zero motion returns the previous pose bit for bit
    assert torch.equal(out[64:70], prev32[64:70])
    # single-pose form
    one = ops.pose_exp_compose(prev32[5].to(gpu), raw32[5].to(gpu)).cpu()
    assert one.shape == (7,) and torch.equal(one, out[5])


# ---------------------------------------------------------------------------------------------- the hot path with a stand-in PoseNet
class _StandInNet:
    """Seeded stand-in for the PoseNet: per-plane means of the [L,5,112,160] input through a fixed 6x5 matrix (clamped first: the
    depth plane may hold FLT_MAX-derived values).  Records its inputs and outputs."""

    def __init__(self, dev, seed=7, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        self.A = (torch.randn(6, 5, generator=g) * 0.5 * scale).to(dev)
        self.b = (torch.randn(6, generator=g) * 0.3 * scale).to(dev)
        self.inputs, self.outputs = [], []

    def __call__(self, x):
        m = torch.tanh(x.clamp(-1e3, 1e3).mean(dim=(2, 3)))
        out = m @ self.A.T + self.b
        self.inputs.append(x.clone())
        self.outputs.append(out.clone())
        return out


def _seq(n_frames, seed=3, H=192, W=256):
    from tests import synth

    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=64, iters=3, seed=seed)
    return cam, frames


def _ins(frames, dev):
    from macvo_amd.pipeline import FrameInputs

    return [FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}) for fr in frames]


def test_zero_motion_net_is_the_static_pipe_bitwise(gpu):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig

    cam, frames = _seq(5)
    zero = lambda x: torch.zeros(x.shape[0], 6, device=x.device)   # noqa: E731
    st = HotPath(Camera(**cam), HotPathConfig(), gpu)
    mo = HotPath(Camera(**cam), HotPathConfig(motion_model="tartan"), gpu, pose_net=zero)
    ins = _ins(frames, gpu)
    st.initialize(ins[0])
    mo.initialize(ins[0])
    for t in range(1, len(ins)):
        torch.manual_seed(40 + t)
        a = st.step(ins[t])
        torch.manual_seed(40 + t)
        b = mo.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(a.kp0_uv, b.kp0_uv) and torch.equal(_bits(a.pose), _bits(b.pose)), t
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info), t
        assert b.prior is not None and a.prior is None


def _oracle_with_prior(ora, monkeypatch, priors):
    """OracleHotPath's step with the motion-model prior substituted: LM starts from priors[-1] (world registration keeps ora.pose), and a
    lost-track frame keeps it."""
    from oracle import pipeline as opl

    real = opl.pgo.PGOProblem

    def problem(**kw):
        kw["init_pose"] = priors[-1].clone()
        return real(**kw)
    monkeypatch.setattr(opl.pgo, "PGOProblem", problem)


def test_sequence_matches_oracle_with_prior(gpu, monkeypatch):
    """HotPath(motion_model="tartan") with a seeded stand-in net against the oracle's loop with the prior substituted, over 6 frames:
    keypoints bit-exact, the prior is prev @ Exp(net * pose_norm) (mv_pose_exp_compose on the previous pose), poses within 1e-4 of the
    oracle at the same LM step count; run() gives step()'s bits."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    n_frames = 6
    cam, frames = _seq(n_frames, seed=5)
    net = _StandInNet(gpu)
    cfg = HotPathConfig(graph_type="icp", motion_model="tartan")
    hot = HotPath(Camera(**cam), cfg, gpu, pose_net=net)
    ora = OracleHotPath(cam, dict(graph_type="icp"))
    priors = []
    _oracle_with_prior(ora, monkeypatch, priors)
    ins = _ins(frames, gpu)
    ora.initialize(frames[0])
    hot.initialize(ins[0])
    poses = []
    for t in range(1, n_frames):
        prev = hot.pose.clone()
        torch.manual_seed(100 + t)
        rh = hot.step(ins[t])
        torch.cuda.synchronize()
        raw = net.outputs[-1]
        assert torch.equal(_bits(rh.prior), _bits(ops.pose_exp_compose(prev, raw.reshape(6)))), t
        # the net saw the frame's temporal flow and depth through mv_motion_input_lanes
        m1 = hot.maps_prev_for_next
        want = ops.motion_input(m1.flow, m1.depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["baseline"])
        assert torch.equal(_bits(net.inputs[-1]), _bits(want)), t
        priors.append(rh.prior.cpu())
        torch.manual_seed(100 + t)
        ro = ora.step(frames[t])
        assert torch.equal(rh.kp0_uv.cpu(), ro["kp0_uv"]), t
        assert int(rh.n_valid.item()) == ro["n_valid"]
        dt, dr = se3.pose_error(ro["pose"].double(), rh.pose.cpu().double())
        assert dt <= 1e-4 and dr <= 1e-4, (t, dt, dr)
        assert int(rh.info[0, 1].item()) == ro["steps"], t
        poses.append(rh.pose.clone())
    # the motion moved the prior away from the previous pose (the test is not the static pipe in disguise)
    assert (priors[-1] - poses[-2].cpu()).abs().max() > 1e-3
    # run(): the software-pipelined loop calls the net between enqueue and finish and computes step()'s bits (one seed for the whole
    # sequence in both: the keypoint draws consume torch's global generator frame after frame)
    hot2 = HotPath(Camera(**cam), cfg, gpu, pose_net=_StandInNet(gpu))
    hot3 = HotPath(Camera(**cam), cfg, gpu, pose_net=_StandInNet(gpu))
    hot2.initialize(ins[0])
    hot3.initialize(ins[0])
    torch.manual_seed(321)
    outs = [r.pose for r in hot2.run(ins[1:])]     # (each frame's pose is its own tensor: valid once run() has synced)
    torch.manual_seed(321)
    steps = [hot3.step(x).pose for x in ins[1:]]
    torch.cuda.synchronize()
    assert len(outs) == len(steps) == n_frames - 1
    for a, b in zip(outs, steps):
        assert torch.equal(_bits(a), _bits(b))


def test_lost_track_keeps_the_prior_and_the_next_prior_composes_onto_it(gpu):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig

    cam, frames = _seq(4, seed=9)
    net = _StandInNet(gpu, seed=3)
    hot = HotPath(Camera(**cam), HotPathConfig(motion_model="tartan", min_num_point=100000), gpu, pose_net=net)
    ins = _ins(frames, gpu)
    hot.initialize(ins[0])
    prev = hot.pose.clone()
    for t in range(1, len(ins)):
        torch.manual_seed(10 + t)
        r = hot.step(ins[t])
        torch.cuda.synchronize()
        want = ops.pose_exp_compose(prev, net.outputs[-1].reshape(6))
        assert torch.equal(_bits(r.prior), _bits(want)), t
        assert torch.equal(_bits(r.pose), _bits(want)), t        # lost track: the frame keeps its prior (MACVO.py:303-307)
        assert int(r.info[0, 1].item()) == 0
        prev = r.pose.clone()
    assert (prev - torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu)).abs().max() > 1e-3


def test_tartan_needs_a_pose_net(gpu):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig

    cam, frames = _seq(2, seed=9)
    hot = HotPath(Camera(**cam), HotPathConfig(motion_model="tartan"), gpu)
    ins = _ins(frames, gpu)
    hot.initialize(ins[0])
    with pytest.raises(ops.L.MacvoHipError):
        hot.step(ins[1])
    with pytest.raises(ops.L.MacvoHipError):
        HotPath(Camera(**cam), HotPathConfig(motion_model="gt"), gpu)


def test_plugin_against_restated_predict_update(gpu):
    """HIP_TartanMotionNet with an injected net against the restated predict / update (torch on the device) over 6 frames: the net's
    input bit for bit, the predicted poses at fp32 roundoff (the restatement composes through the PyPose shim)."""
    from types import SimpleNamespace

    from macvo_amd import plugins

    H, W = 240, 333
    K = (CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["baseline"])
    frame = SimpleNamespace(stereo=SimpleNamespace(fx=K[0], fy=K[1], cx=K[2], cy=K[3], frame_baseline=K[4], height=H, width=W))
    net_h, net_r = _StandInNet(gpu, seed=11), _StandInNet(gpu, seed=11)
    mm = plugins.HIP_TartanMotionNet(SimpleNamespace(weight="", device="cuda"), pose_net=net_h)
    ref = R.MotionModelRef(net_r, pp, gpu)
    p_h = mm.predict(frame, None, None)
    p_r = ref.predict(None, None, *K)
    assert torch.equal(torch.as_tensor(p_h).reshape(7), p_r)
    for k in range(1, 7):
        upd = p_r + torch.tensor([0.01 * k, -0.003, 0.002, 0, 0, 0, 0], device=gpu)
        mm.update(upd)
        ref.update(upd)
        flow, depth = _maps(H, W, 1, 60 + k, special=k % 2 == 0)
        p_h = torch.as_tensor(mm.predict(frame, flow.to(gpu), depth.to(gpu))).reshape(7)
        p_r = ref.predict(flow.to(gpu), depth.to(gpu), *K)
        assert torch.equal(_bits(net_h.inputs[-1]), _bits(net_r.inputs[-1])), k
        assert (p_h - p_r).abs().max() <= 64 * 2.0 ** -23, k
