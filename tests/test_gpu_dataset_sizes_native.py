"""KITTI- and EuRoC-sized frames (376 x 784: the 780-wide KITTI frame padded to a multiple of 8 as FlowFormer's InputPadder does; 480 x 752) through
the hot paths: 1/8 maps of 47 x 98 and 60 x 94 pixels, N = 4606 / 5640 — no multiples of 64.  The native frame driver and the Python-sequenced HotPath run
the packed streaming volume (ragged last sub-tile) and agree bit for bit; the poses follow the CPU oracle; Fast mode stores 2-byte cells."""
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu

SIZES = [(376, 784), (480, 752)]


def _to(fr, dev):
    from macvo_amd.pipeline import FrameInputs

    return FrameInputs(**{k: (None if v is None else v.to(dev)) for k, v in fr.items()})


@pytest.mark.parametrize("H,W", SIZES)
def test_native_driver_equals_hotpath_and_follows_the_oracle(gpu, H, W):
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, HotPath, HotPathConfig, NativeHotPath
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    n_frames = 3
    cam, frames, _ = synth.make_sequence(n_frames, H, W, C=256, iters=2, seed=31)
    ins = [_to(fr, gpu) for fr in frames]
    torch.cuda.synchronize()
    py = HotPath(Camera(**cam), HotPathConfig(), gpu, keep_extras=True)
    nat = NativeHotPath(Camera(**cam), HotPathConfig(), gpu, keep_extras=True)
    ora = OracleHotPath(cam, {})
    assert py.cfg.volume_precision == "f16x2"
    py.initialize(ins[0])
    nat.initialize(ins[0])
    ora.initialize(frames[0])
    for t in range(1, n_frames):
        torch.manual_seed(500 + t)
        ro = ora.step(frames[t])
        torch.manual_seed(500 + t)
        a = py.step(ins[t])
        torch.cuda.synchronize()
        assert ops.last_volume_kernel() == "corr_volume_split_stream<f16x2>", ops.last_volume_kernel()
        torch.manual_seed(500 + t)
        b = nat.step(ins[t])
        torch.cuda.synchronize()
        assert ops.last_volume_kernel() == "corr_volume_split_stream<f16x2>", ops.last_volume_kernel()
        # the driver against the Python-sequenced path, as tests/test_gpu_native.py compares them
        assert torch.equal(py.last_tokens, nat.last_tokens)
        ma, mb = py.maps_prev_for_next, nat.maps()
        for f in ("depth", "depth_cov", "disparity", "disparity_cov", "flow", "flow_cov"):
            assert torch.equal(getattr(ma, f), getattr(mb, f)), f
        assert torch.equal(a.kp0_uv, b.kp0_uv), t
        assert torch.equal(a.n_valid, b.n_valid)
        for k in ("cov0", "cov0_w", "cov1", "valid", "pos_Tw"):
            assert torch.equal(a.extras[k], b.extras[k]), k
        assert torch.equal(a.pose_f64, b.pose_f64) and torch.equal(a.info, b.info)
        assert torch.equal(a.pose, b.pose), t
        # ... and against the CPU oracle
        torch.testing.assert_close(nat.last_tokens.cpu(), ora.last_tokens, rtol=1e-5, atol=3e-4)
        assert torch.equal(b.kp0_uv.cpu(), ro["kp0_uv"]), t
        d_t, d_r = se3.pose_error(ro["pose"].double(), b.pose.cpu().double())
        assert d_t <= 1e-4 and d_r <= 1e-4, (t, d_t, d_r)


def test_fast_mode_stores_two_byte_cells_at_376x784(gpu):
    """fp16 HWC features, `volume_store="encoder"`: the driver's volume is `corr_volume_h_stream<out16>` at N = 4606 too (row-major: 98 columns are no
    multiple of 4, so the tiled lookup stays off), tokens / keypoints / pose as tests/test_gpu_fastmode.py states them at 640 x 480"""
    from macvo_amd import ops
    from macvo_amd.pipeline import Camera, FrameInputs, HotPathConfig, NativeHotPath
    from oracle import se3
    from oracle.pipeline import OracleHotPath

    cam, frames, _ = synth.make_sequence(3, 376, 784, C=256, iters=2, seed=21)
    fr16 = [dict(fr, fmap1=fr["fmap1"].permute(0, 2, 3, 1).contiguous().half(), fmap2=fr["fmap2"].permute(0, 2, 3, 1).contiguous().half()) for fr in frames]
    fr_cpu = [dict(fr, fmap1=fr["fmap1"].half().float(), fmap2=fr["fmap2"].half().float()) for fr in frames]
    ora = OracleHotPath(cam, dict(volume_store="encoder"))
    hot = NativeHotPath(Camera(**cam), HotPathConfig(feature_layout="hwc", volume_store="encoder"), gpu)
    ins = [FrameInputs(**{k: v.to(gpu) for k, v in fr.items()}) for fr in fr16]
    torch.cuda.synchronize()
    ora.initialize(fr_cpu[0])
    hot.initialize(ins[0])
    assert not hot.volume_tiled
    for t in (1, 2):
        torch.manual_seed(70 + t)
        ro = ora.step(fr_cpu[t])
        torch.manual_seed(70 + t)
        rh = hot.step(ins[t])
        torch.cuda.synchronize()
        assert ops.last_volume_kernel() == "corr_volume_h_stream<out16>", ops.last_volume_kernel()
        tok, ref_tok = hot.last_tokens.cpu(), ora.last_tokens
        assert (tok - ref_tok).abs().max().item() <= 2.0 ** -10 * max(1.0, ref_tok.abs().max().item())
        assert ((tok - ref_tok).abs() > 3e-4).float().mean().item() < 0.02
        assert torch.equal(rh.kp0_uv.cpu(), ro["kp0_uv"])
        dt, dr = se3.pose_error(ro["pose"].double(), rh.pose.cpu().double())
        assert dt <= 1e-4 and dr <= 1e-4, (t, dt, dr)
