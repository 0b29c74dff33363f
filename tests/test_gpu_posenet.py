"""GPU: the PoseNet forward in HIP (``ops.PoseNet`` / ``mv_posenet_forward_lanes``) — output and all six stages against the fp64 torch
restatement, bit for bit against the host twin, lane independence, repeatability, NaN / inf propagation, and as the ``pose_net`` of
``HotPath``, ``NativeHotPath`` and the ``HIP_TartanMotionNet_HIPPoseNet`` plugin.

Tolerance: with E(y) = max|y - y64| / max|y64| against the fp64 restatement, E <= 16 x E(torch's fp32 CPU forward of the same case), per
tensor, computed here (tests/posenet_twin.py).  The shape is fixed by the network; its own 7x10 -> 4x5 -> 2x3 maps are the small, odd cases."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

from tests import posenet_twin as T
from tests import synth
from tools import posenet_torch as PT

pytestmark = pytest.mark.gpu

CANARY = 64          # trailing words of out / stage buffers that must survive
CANARY_VALUE = -12345.5


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def nets(gpu):
    from macvo_amd import ops

    return {seed: ops.PoseNet.from_state_dict(T.case(seed, 3)[0], gpu) for seed in T.WEIGHT_SEEDS}


@pytest.mark.parametrize("seed", T.WEIGHT_SEEDS)
@pytest.mark.parametrize("lanes", [1, 3])
def test_forward_and_stages_against_fp64(gpu, nets, seed, lanes):
    """The C entry point on a NaN-filled workspace, with canaries behind out and every stage buffer."""
    from macvo_amd import _lib as L
    from macvo_amd import ops

    lib = L.load()
    ref = T.case(seed, lanes)
    x = ref[1].to(gpu)
    ws = torch.full((lib.mv_posenet_workspace_bytes(lanes) // 4,), float("nan"), device=gpu)
    sizes = [lanes * 6] + [lanes * c * h * w for c, h, w in ops.POSENET_STAGE_SHAPES]
    bufs = [torch.full((n + CANARY,), CANARY_VALUE, device=gpu) for n in sizes]
    sp = (C.c_void_p * 6)(*[b.data_ptr() for b in bufs[1:]])
    L.check(lib.mv_posenet_forward_lanes(nets[seed].packed.data_ptr(), x.data_ptr(), lanes, bufs[0].data_ptr(), ws.data_ptr(), sp, ops._stream()),
            "mv_posenet_forward_lanes")
    torch.cuda.synchronize()
    for b, n in zip(bufs, sizes):
        assert bool((b[n:] == CANARY_VALUE).all()), "a canary behind an output buffer was overwritten"
    y = bufs[0][:sizes[0]].reshape(lanes, 6).cpu()
    stages = [b[:n].reshape((lanes,) + s).cpu() for b, n, s in zip(bufs[1:], sizes[1:], ops.POSENET_STAGE_SHAPES)]
    T.check_against_fp64(f"kernel, seed {seed}, {lanes} lane(s)", y, stages, ref)
    # the wrapper (its own workspace, stages on request) returns the same bits
    y2, st2 = nets[seed](x, return_stages=True)
    assert torch.equal(_bits(y2.cpu()), _bits(y)) and all(torch.equal(_bits(a.cpu()), _bits(b)) for a, b in zip(st2, stages))
    assert torch.equal(_bits(nets[seed](x)), _bits(y2))


def test_kernel_equals_the_host_twin_bit_for_bit(gpu, nets):
    """The fp32 MFMA is a k-ordered fmaf chain: the kernel's output and stages are the host replay's bits (measured on MI355X: 0 ulp on all seven)."""
    seed = T.WEIGHT_SEEDS[0]
    sd, x = T.case(seed, 1)[:2]
    ty, tst = T.forward(T.pack(sd), x)
    y, st = nets[seed](x.to(gpu), return_stages=True)
    for name, a, b in zip(("out",) + PT.STAGES, [ty] + tst, [y] + st):
        ulp = int((_bits(a).long() - _bits(b.cpu()).long()).abs().max())
        print(f"[posenet] kernel vs twin, {name}: max distance {ulp} ulp")
        assert torch.equal(_bits(a), _bits(b.cpu())), f"{name}: kernel and host twin differ by up to {ulp} ulp"


def test_a_lanes_bits_do_not_depend_on_the_batch(gpu, nets):
    net = nets[T.WEIGHT_SEEDS[0]]
    g = torch.Generator().manual_seed(17)
    x5 = torch.randn(5, 5, 112, 160, generator=g).to(gpu)
    y5, st5 = net(x5, return_stages=True)
    for l in range(5):
        y1, st1 = net(x5[l:l + 1].contiguous(), return_stages=True)
        assert torch.equal(_bits(y1), _bits(y5[l:l + 1])), l
        assert all(torch.equal(_bits(a), _bits(b[l:l + 1])) for a, b in zip(st1, st5)), l
    x64 = torch.randn(64, 5, 112, 160, generator=g).to(gpu)
    y64 = net(x64)
    for l in (0, 63):
        assert torch.equal(_bits(net(x64[l:l + 1].contiguous())), _bits(y64[l:l + 1])), l


def test_two_runs_give_the_same_bits(gpu, nets):
    net = nets[T.WEIGHT_SEEDS[1]]
    x = T.case(T.WEIGHT_SEEDS[1], 3)[1].to(gpu)
    a, sa = net(x, return_stages=True)
    b, sb = net(x, return_stages=True)
    assert torch.equal(_bits(a), _bits(b)) and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(sa, sb))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nan_and_inf_stay_in_their_lane(gpu, nets, bad):
    """One NaN (or +inf) at one pixel of the depth channel of lane 1: all six outputs of lane 1 are NaN (non-finite for +inf), as torch's are;
    lanes 0 and 2 keep the clean run's bits."""
    seed = T.WEIGHT_SEEDS[0]
    net = nets[seed]
    x = T.case(seed, 3)[1].clone()
    clean = net(x.to(gpu))
    x[1, 2, 57, 83] = bad
    y = net(x.to(gpu))
    with torch.no_grad():
        yt = PT.from_state_dict(T.case(seed, 3)[0])(x[1:2])
    if math.isnan(bad):
        assert bool(torch.isnan(yt).all()) and bool(torch.isnan(y[1]).all())
    else:
        assert not bool(torch.isfinite(yt).any()) and not bool(torch.isfinite(y[1]).any())
    assert torch.equal(_bits(y[0]), _bits(clean[0])) and torch.equal(_bits(y[2]), _bits(clean[2]))


# ------------------------------------------------------------------------------------------------------- as the hot paths' pose_net
class _Recorder:
    """A pose_net that records what it was given and what it returned."""

    def __init__(self, net):
        self.net, self.inputs, self.outputs = net, [], []

    def __call__(self, x):
        y = self.net(x)
        self.inputs.append(x.clone())
        self.outputs.append(y.clone())
        return y


class _Restated64:
    """The eager restatement as a pose_net: fp64 on the CPU (the tolerance's reference), returned as fp32 on the device."""

    def __init__(self, sd, dev):
        self.net64, self.net32, self.dev = PT.from_state_dict(sd, dtype=torch.float64), PT.from_state_dict(sd), dev
        self.y64, self.e32 = [], []

    def __call__(self, x):
        xc = x.detach().cpu()
        with torch.no_grad():
            y64 = self.net64(xc.double())
            self.e32.append(T.rel_err(self.net32(xc), y64))
        self.y64.append(y64)
        return y64.float().to(self.dev)


def _ins(frames, dev):
    from macvo_amd.pipeline import FrameInputs

    return [FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}) for fr in frames]


@pytest.mark.parametrize("driver,lanes", [("python", 1), ("native", 1), ("native", 2)])
def test_posenet_as_the_hot_paths_pose_net(gpu, nets, driver, lanes):
    """4 frames at 240 x 320: the raw motion the compose receives is ops.PoseNet on the frame's MOTION_IN, bit for bit (prior = previous pose @
    Exp(raw * pose_norm) with that raw); poses are finite; a run with the restatement as pose_net sees the same inputs and its fp64 raw motions
    are met within the tolerance."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath, stack_lanes

    seed, n_frames = T.WEIGHT_SEEDS[0], 5
    seqs = [synth.make_sequence(n_frames, 240, 320, C=64, iters=2, seed=41 + 13 * l) for l in range(lanes)]
    cam = seqs[0][0]
    per_lane = [_ins(s[1], gpu) for s in seqs]
    frames = [stack_lanes([per_lane[l][t] for l in range(lanes)]) if lanes > 1 else per_lane[0][t] for t in range(n_frames)]
    cfg = HotPathConfig(graph_type="icp", motion_model="tartan")

    def run(net):
        if driver == "python":
            hot = HotPath(Camera(**cam), cfg, gpu, pose_net=net)
        else:
            hot = NativeHotPath(Camera(**cam), cfg, gpu, lanes=lanes, generators=[torch.Generator().manual_seed(3 + l) for l in range(lanes)], pose_net=net)
        hot.initialize(frames[0])
        priors, poses = [], []
        for t in range(1, n_frames):
            torch.manual_seed(500 + t)
            res = hot.step(frames[t])
            torch.cuda.synchronize()
            rs = res if isinstance(res, list) else [res]
            priors.append(torch.stack([r.prior.reshape(7).clone() for r in rs]))
            poses.append(torch.stack([r.pose.reshape(7).clone() for r in rs]))
        if driver == "native":
            hot.close()
        return priors, poses

    rec = _Recorder(nets[seed])
    priors, poses = run(rec)
    assert len(rec.inputs) == n_frames - 1
    prev = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=gpu).repeat(lanes, 1)
    for t, (x, raw) in enumerate(zip(rec.inputs, rec.outputs)):
        assert x.shape == (lanes, 5, 112, 160)
        assert torch.equal(_bits(nets[seed](x)), _bits(raw)), t
        assert torch.equal(_bits(priors[t]), _bits(ops.pose_exp_compose(prev, raw.reshape(lanes, 6)))), t
        assert bool(torch.isfinite(poses[t]).all()) and bool(torch.isfinite(priors[t]).all()), t
        prev = poses[t]
    eager = _Recorder(_Restated64(T.case(seed, 3)[0], gpu))
    run(eager)
    for t in range(n_frames - 1):
        assert torch.equal(_bits(eager.inputs[t]), _bits(rec.inputs[t])), t      # MOTION_IN comes from the frontend alone
        y64, bar = eager.net.y64[t], T.TOL_FACTOR * eager.net.e32[t]
        e = T.rel_err(rec.outputs[t], y64)
        print(f"[posenet] {driver} x{lanes} frame {t + 1}: raw motion E={e:.2e}, bar 16 x {eager.net.e32[t]:.2e}")
        assert e <= bar, (t, e, bar)


def test_plugin_with_the_hip_posenet(gpu, tmp_path):
    """HIP_TartanMotionNet_HIPPoseNet over a temporary release-layout checkpoint against HIP_TartanMotionNet(pose_net = the fp64 restatement):
    predict / update over 3 frames.  With d = 16 x E(torch fp32 CPU) x max|raw64| the bound on a raw component, the tangent moves by at most
    0.13 d per translation and 0.013 d per rotation component; through Exp and the compose the translation moves by at most
    sqrt(3) (0.13 d + 0.5 * 0.013 d |rho|) (|V| <= 1, |dV| <= |dphi| / 2, rho = the translation tangent) and the quaternion by sqrt(3) 0.013 d / 2;
    the bound below takes sqrt(3) * 0.13 d (1 + |rho|), which covers both, plus 64 ulp of the pose's magnitude for the fp32 compose."""
    from macvo_amd import interfaces as I
    from macvo_amd import ops, plugins
    from macvo_amd.pipeline import hip_pose_net, motion_config_fields

    seed = T.WEIGHT_SEEDS[1]
    sd = T.case(seed, 3)[0]
    ck = {"module.flowPoseNet." + k: v for k, v in sd.items()}
    ck["module.flowNet.moduleExtractor.weight"] = torch.zeros(3, 3)
    path = str(tmp_path / "MACVO_posenet.pkl")
    torch.save(ck, path)
    assert I.IMotionModel.get_class("HIP_TartanMotionNet_HIPPoseNet") is plugins.HIP_TartanMotionNet_HIPPoseNet
    assert motion_config_fields({"type": "HIP_TartanMotionNet_HIPPoseNet", "args": {}}) == {"motion_model": "tartan"}
    with pytest.raises(ops.L.MacvoHipError, match="weight"):
        plugins.HIP_TartanMotionNet_HIPPoseNet(SimpleNamespace(weight="", device="cuda"))
    mm = plugins.HIP_TartanMotionNet_HIPPoseNet(SimpleNamespace(weight=path, device="cuda"))
    assert isinstance(mm.net, ops.PoseNet) and torch.equal(mm.net.packed, hip_pose_net(path, gpu).packed)
    eager = _Restated64(sd, gpu)
    mr = plugins.HIP_TartanMotionNet(SimpleNamespace(weight="", device="cuda"), pose_net=eager)

    H, W = 240, 320
    frame = SimpleNamespace(stereo=SimpleNamespace(fx=160.0, fy=161.0, cx=159.5, cy=119.5, frame_baseline=0.25, height=H, width=W))
    p_h = torch.as_tensor(mm.predict(frame, None, None)).reshape(7)
    p_r = torch.as_tensor(mr.predict(frame, None, None)).reshape(7)
    assert torch.equal(p_h, p_r)
    g = torch.Generator().manual_seed(77)
    for k in range(1, 4):
        upd = p_r + torch.tensor([0.01 * k, -0.003, 0.002, 0, 0, 0, 0], device=gpu)
        mm.update(upd)
        mr.update(upd)
        flow = (torch.randn(1, 2, H, W, generator=g) * 2).to(gpu)
        depth = (torch.rand(1, 1, H, W, generator=g) * 10 + 2).to(gpu)
        p_h = torch.as_tensor(mm.predict(frame, flow, depth)).reshape(7)
        p_r = torch.as_tensor(mr.predict(frame, flow, depth)).reshape(7)
        y64 = eager.y64[-1]
        d = T.TOL_FACTOR * eager.e32[-1] * float(y64.abs().max())
        rho = float(y64[0, :3].abs().max()) * 0.13 * math.sqrt(3)
        tol = math.sqrt(3) * 0.13 * d * (1 + rho) + 64 * 2.0 ** -23 * max(1.0, float(p_r.abs().max()))
        err = float((p_h - p_r).abs().max())
        print(f"[posenet] plugin frame {k}: pose differs by {err:.2e}, bound {tol:.2e}")
        assert bool(torch.isfinite(p_h).all()) and err <= tol, (k, err, tol)
