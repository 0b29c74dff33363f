"""Frames whose sides are no multiples of 8 through the hot paths, un-padded as the network's InputPadder leaves them: KITTI's 376 x 780 (47 x 98 maps at
1/8 resolution), 237 x 315 (pads 3 and 5: odd rows, odd planes) and 236 x 316 (even pads).  Dense fields live on the H x W frame, feature maps / coords /
1/8-resolution fields on ceil(H / 8) x ceil(W / 8) (tests/unpad_ref.py).  The native driver and the Python-sequenced HotPath agree bit for bit, the poses
follow the CPU oracle — with the bars of tests/test_gpu_dataset_sizes_native.py."""
import pytest
import torch

from tests import unpad_ref

pytestmark = pytest.mark.gpu

SIZES = [(236, 316, 64), (237, 315, 64), (376, 780, 32)]
MAPS = ("depth", "depth_cov", "disparity", "disparity_cov", "flow", "flow_cov")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _to(fr, dev, **kw):
    from macvo_amd.pipeline import FrameInputs

    return FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()}, **kw)


def _pair(cam, cfg_kw, dev, **kw):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    return (HotPath(Camera(**cam), HotPathConfig(**cfg_kw), dev, keep_extras=True, **kw),
            NativeHotPath(Camera(**cam), HotPathConfig(**cfg_kw), dev, keep_extras=True, **kw))


def _same_step(py, nat, a, b, t):
    """NativeHotPath's frame against HotPath's, as tests/test_gpu_native.py compares them."""
    assert torch.equal(py.last_tokens, nat.last_tokens)
    ma, mb = py.maps_prev_for_next, nat.maps()
    for f in MAPS:
        assert getattr(mb, f).shape[-2:] == (nat.cam.H, nat.cam.W)
        assert torch.equal(getattr(ma, f), getattr(mb, f)), f
    assert torch.equal(a.kp0_uv, b.kp0_uv), t
    assert torch.equal(a.n_valid, b.n_valid)
    for k in ("cov0", "cov0_w", "cov1", "valid", "pos_Tw"):
        assert torch.equal(a.extras[k], b.extras[k]), k
    for f in ("kp0_uv", "kp1_uv", "inbound", "vals", "sigma0", "sigma1"):
        assert torch.equal(getattr(a.extras["tracked"], f), getattr(b.extras["tracked"], f)), f
    assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info)
    assert torch.equal(a.pose, b.pose), t


@pytest.mark.parametrize("H,W,C", SIZES)
def test_unpadded_frames_native_equals_hotpath_and_follows_the_oracle(gpu, H, W, C):
    """`flow` / `logcov` at H x W as `inference` returns them next to feature maps of the padded size."""
    from macvo_amd import ops
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    n_frames = 3
    cam, frames, _ = unpad_ref.make_sequence(n_frames, H, W, C=C, iters=2, seed=31)
    ins = [_to(fr, gpu) for fr in frames]
    torch.cuda.synchronize()
    py, nat = _pair(cam, {}, gpu)
    ora = OracleHotPath(cam, {})
    py.initialize(ins[0])
    nat.initialize(ins[0])
    ora.initialize(frames[0])
    for t in range(1, n_frames):
        torch.manual_seed(500 + t)
        ro = ora.step(frames[t])
        torch.manual_seed(500 + t)
        a = py.step(ins[t])
        torch.manual_seed(500 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert nat.last_tokens.shape[-2:] == ops.eighth_shape(H, W) == (-(-H // 8), -(-W // 8))
        _same_step(py, nat, a, b, t)
        torch.testing.assert_close(nat.last_tokens.cpu(), ora.last_tokens, rtol=1e-5, atol=3e-4)
        assert torch.equal(b.kp0_uv.cpu(), ro["kp0_uv"]), t
        d_t, d_r = se3.pose_error(ro["pose"].double(), b.pose.cpu().double())
        assert d_t <= 1e-4 and d_r <= 1e-4, (t, d_t, d_r)
    nat.close()


@pytest.mark.parametrize("H,W,C", [(237, 315, 64), (376, 780, 32)])
def test_unpadded_upsample_path(gpu, H, W, C):
    """`flow8` / `cov8` / masks at h8 x w8: both hot paths upsample straight into the un-padded window (mv_convex_upsample_crop) — the bits of a HotPath that is
    handed the crops of the padded upsampling — and the pose follows the oracle fed the same crops of its own `upsample_flow`."""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig
    from oracle import frontend, se3
    from oracle.pipeline import OracleHotPath

    n_frames = 3
    _, _, y0, x0 = unpad_ref.pad_of(H, W)
    cam, frames, _ = unpad_ref.make_sequence(n_frames, H, W, fields8=True, C=C, iters=2, seed=9)
    ins = [_to(fr, gpu) for fr in frames]
    crop = lambda t: t[..., y0: y0 + H, x0: x0 + W].contiguous()  # noqa: E731
    ins_c = [_to(dict(fmap1=fr["fmap1"], fmap2=fr["fmap2"], coords=fr["coords"]), gpu, cov_is_log=False,
                 flow=crop(ops.convex_upsample(x.flow8, x.up_mask, 0.25)), logcov=crop(ops.convex_upsample(x.cov8, x.cov_mask, 1.0, True)))
             for fr, x in zip(frames, ins)]
    fr_o = [dict(fmap1=fr["fmap1"], fmap2=fr["fmap2"], coords=fr["coords"], flow=crop(frontend.upsample_flow(fr["flow8"], 0.25 * fr["up_mask"])),
                 cov_exp=crop(torch.exp(frontend.upsample_flow(fr["cov8"], fr["cov_mask"]) * 2))) for fr in frames]
    torch.cuda.synchronize()
    py, nat = _pair(cam, {}, gpu)
    pyc = HotPath(Camera(**cam), HotPathConfig(), gpu, keep_extras=True)
    ora = OracleHotPath(cam, {})
    py.initialize(ins[0])
    nat.initialize(ins[0])
    pyc.initialize(ins_c[0])
    ora.initialize(fr_o[0])
    for t in range(1, n_frames):
        torch.manual_seed(40 + t)
        ro = ora.step(fr_o[t])
        torch.manual_seed(40 + t)
        a = py.step(ins[t])
        torch.manual_seed(40 + t)
        b = nat.step(ins[t])
        torch.manual_seed(40 + t)
        c = pyc.step(ins_c[t])
        torch.cuda.synchronize()
        _same_step(py, nat, a, b, t)
        mb, mc = nat.maps(), pyc.maps_prev_for_next
        for f in MAPS:
            assert torch.equal(getattr(mb, f), getattr(mc, f)), f
        assert torch.equal(b.kp0_uv, c.kp0_uv) and torch.equal(b.pose_f64, c.pose_f64) and torch.equal(b.pose, c.pose), t
        # (no keypoint bar against the oracle here: the kernel's exp differs from torch's by ~1.5 ulp and may move a candidate across a threshold)
        d_t, d_r = se3.pose_error(ro["pose"].double(), b.pose.cpu().double())
        print(f"[unpadded upsample path {H}x{W}] frame {t}: keypoints equal to the oracle's: {torch.equal(b.kp0_uv.cpu(), ro['kp0_uv'])}, "
              f"pose error {d_t:.3e} m / {d_r:.3e} rad")
        assert d_t <= 1e-4 and d_r <= 1e-4, (t, d_t, d_r)
    nat.close()


def test_two_lanes_at_an_odd_plane_equal_their_solo_runs(gpu):
    """237 x 315: H * W is odd, so the planes of lane 1 (and every second plane of lane 0) start on odd float offsets."""
    from macvo_amd.pipeline import Camera, HotPathConfig, NativeHotPath, stack_lanes

    H, W, n_frames, lanes = 237, 315, 3, 2
    gens = lambda seeds: [torch.Generator().manual_seed(s) for s in seeds]  # noqa: E731
    for fields8 in (False, True):
        seqs = [unpad_ref.make_sequence(n_frames, H, W, fields8=fields8, mask_seed=2 + l, C=64, iters=2, seed=200 + l, pool=1) for l in range(lanes)]
        cam = seqs[0][0]
        hp = NativeHotPath(Camera(**cam), HotPathConfig(), gpu, lanes=lanes, generators=gens([3000 + l for l in range(lanes)]))
        batched = [stack_lanes([_to(seqs[l][1][t], gpu) for l in range(lanes)]) for t in range(n_frames)]
        torch.cuda.synchronize()
        hp.initialize(batched[0])
        got = []
        for t in range(1, n_frames):
            res = hp.step(batched[t])
            torch.cuda.synchronize()
            got.append([(r.kp0_uv.clone(), r.pose.clone(), r.info.clone()) for r in res])
        toks = hp.last_tokens.clone()
        lane_maps = [{f: getattr(hp.maps(lane=l), f).clone() for f in MAPS} for l in range(lanes)]
        hp.close()
        for l in range(lanes):
            solo = NativeHotPath(Camera(**cam), HotPathConfig(), gpu, generators=gens([3000 + l]))
            ins = [_to(fr, gpu) for fr in seqs[l][1]]
            torch.cuda.synchronize()
            solo.initialize(ins[0])
            for t in range(1, n_frames):
                r = solo.step(ins[t])
                torch.cuda.synchronize()
                kp, pose, info = got[t - 1][l]
                assert torch.equal(r.kp0_uv, kp) and torch.equal(r.pose, pose) and torch.equal(r.info, info), (fields8, l, t)
            assert torch.equal(solo.last_tokens, toks[2 * l: 2 * l + 2]), l
            for f in MAPS:
                assert torch.equal(getattr(solo.maps(), f), lane_maps[l][f]), (fields8, l, f)
            solo.close()


def test_full_selector_with_the_mapping_tail_at_237x315(gpu):
    H, W, n_frames = 237, 315, 4
    cam, frames, _ = unpad_ref.make_sequence(n_frames, H, W, C=64, iters=2, seed=23)
    g = torch.Generator().manual_seed(1)
    for fr in frames:
        fr["image"] = torch.rand(3, H, W, generator=g)
    ins = [_to(fr, gpu) for fr in frames]
    torch.cuda.synchronize()
    py, nat = _pair(cam, dict(selector="full", mapping=True, map_max_depth=13.0, map_max_depth_cov=0.5, map_num_point=500), gpu)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    seen = 0
    for t in range(1, n_frames):
        torch.manual_seed(70 + t)
        a = py.step(ins[t])
        torch.manual_seed(70 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        _same_step(py, nat, a, b, t)
        ma, mb = a.map_points, b.map_points
        assert (ma is None) == (mb is None), t
        if mb is not None:
            assert torch.equal(ma.uv, mb.uv) and torch.equal(_bits(ma.pos_Tw), _bits(mb.pos_Tw)) and torch.equal(ma.color, mb.color), t
            assert torch.equal(_bits(ma.depth), _bits(mb.depth)) and torch.equal(ma.cov_Tc, mb.cov_Tc), t
            seen += mb.uv.shape[0]
    assert seen > 0
    nat.close()


class _Net:
    """Fixed stand-in PoseNet: per-plane means of [L, 5, 112, 160] through a seeded 6 x 5 matrix.  Records its inputs."""

    def __init__(self, dev, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.A = (torch.randn(6, 5, generator=g) * 0.5).to(dev)
        self.b = (torch.randn(6, generator=g) * 0.3).to(dev)
        self.inputs = []

    def __call__(self, x):
        self.inputs.append(x.clone())
        return torch.cat([torch.tanh(x[l:l + 1].clamp(-1e3, 1e3).mean(dim=(2, 3))) @ self.A.T + self.b for l in range(x.shape[0])])


def test_tartan_motion_model_at_237x315(gpu):
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath

    H, W, n_frames = 237, 315, 4
    cam, frames, _ = unpad_ref.make_sequence(n_frames, H, W, C=64, iters=2, seed=21)
    ins = [_to(fr, gpu) for fr in frames]
    torch.cuda.synchronize()
    cfg = HotPathConfig(motion_model="tartan")
    na, nb = _Net(gpu), _Net(gpu)
    py = HotPath(Camera(**cam), cfg, gpu, pose_net=na)
    nat = NativeHotPath(Camera(**cam), cfg, gpu, pose_net=nb)
    py.initialize(ins[0])
    nat.initialize(ins[0])
    for t in range(1, n_frames):
        torch.manual_seed(300 + t)
        a = py.step(ins[t])
        torch.manual_seed(300 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert torch.equal(_bits(na.inputs[-1]), _bits(nb.inputs[-1])), t
        assert torch.equal(a.kp0_uv, b.kp0_uv), t
        assert torch.equal(_bits(a.prior), _bits(b.prior)), t
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info), t
        assert torch.equal(_bits(a.pose), _bits(b.pose)), t
    nat.close()
