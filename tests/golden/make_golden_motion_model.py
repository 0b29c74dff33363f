"""Writes tests/golden/motion_model.npz: the reference's OWN TartanMotionNet code on CPU tensors — TartanStereoVOMotion.inference
(Module/Network/TartanVOStereo/StereoVO_Interface.py:158-194, with its cropAndResize, make_device_intrinsic_layer and centerCropTo)
and TartanMotionNet.predict / update (Module/MotionModel.py:90-118) with a seeded stand-in PoseNet.  Build-container only (needs the
reference checkout); imports it through tests.golden.make_golden.import_reference.  The inputs are regenerated from seeds
(:func:`inputs`), so the fixture holds SHA-256 digests of the full PoseNet inputs, a sample of their values and the poses.

    python tests/golden/make_golden_motion_model.py
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, H, W, seed, special depths)
CASES = (("vga", 480, 640, 1, False), ("odd", 485, 651, 2, True), ("special", 240, 333, 3, True))
CAM = dict(fx=320.0, fy=321.5, cx=319.5, cy=239.25, baseline=0.25)
SEQ_FRAMES, SEQ_H, SEQ_W = 6, 240, 320
SAMPLE = 512


def inputs(H, W, seed, special):
    """flow [1,2,H,W], depth [1,1,H,W] fp32: smooth fields + noise; ``special`` scatters NaN, 0, negative and +-inf depths and puts
    blocks of them where the bilinear taps straddle their edges."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    flow = torch.stack([3 * xx + yy, -2 * yy + 0.5 * xx], 0)[None] + torch.randn(1, 2, H, W, generator=g)
    depth = (2.0 + 10 * (xx + 1) * (yy + 1.5) + torch.rand(H, W, generator=g))[None, None].contiguous()
    if special:
        flat = depth.view(-1)
        idx = torch.randperm(H * W, generator=g)[: H * W // 40]
        q = idx.numel() // 5
        flat[idx[:q]] = float("nan")
        flat[idx[q:2 * q]] = 0.0
        flat[idx[2 * q:3 * q]] = -2.5
        flat[idx[3 * q:4 * q]] = float("inf")
        flat[idx[4 * q:]] = -float("inf")
        depth[..., H // 2: H // 2 + 9, W // 3: W // 3 + 13] = 0.0
        depth[..., H // 3: H // 3 + 7, W // 2: W // 2 + 5] = float("nan")
        depth[..., H // 4: H // 4 + 5, W // 4: W // 4 + 6] = -1.0
    return flow.float().contiguous(), depth.float()


class StandInPoseNet:
    """A seeded deterministic stand-in for StereoVONet.flowPoseNet: per-channel means of the [1,5,112,160] input through a fixed
    6x5 matrix (NaN-free: the depth channel may hold FLT_MAX-derived values, so it is squashed first)."""

    def __init__(self, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.A = torch.randn(6, 5, generator=g) * 0.5
        self.b = torch.randn(6, generator=g) * 0.2

    def __call__(self, x, scale_disp=1.0):
        m = torch.tanh(x.float().clamp(-1e3, 1e3).mean(dim=(2, 3)))        # [n, 5]
        return (m @ self.A.T + self.b).reshape(x.shape[0], 6)


def seq_inputs(k):
    return inputs(SEQ_H, SEQ_W, 100 + k, k % 2 == 1)


def seq_update(pose, k):
    """What the optimizer hands back to update() after frame k (a deterministic nudge of the prediction)."""
    d = torch.tensor([0.01 * (k + 1), -0.004 * k, 0.002, 0, 0, 0, 0], dtype=torch.float32)
    return pose + d


def sha(t: torch.Tensor) -> str:
    import hashlib

    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def sample_idx(n, seed=0):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:SAMPLE]


def main():
    from tests.golden import make_golden as MG

    MG.import_reference()
    import Module.MotionModel as MM
    import pypose as pp
    from tests.golden import pypose_shim

    pp.se3 = lambda d: pypose_shim.LieTensor(d, ltype="se3")   # (PyPose's se3 constructor: the shim's tangent type)
    from Module.Network.TartanVOStereo.StereoVO_Interface import TartanStereoVOMotion

    captured = []
    net = StandInPoseNet()

    def flow_pose_net(x, scale_disp=1.0):
        captured.append(x.clone())
        return net(x, scale_disp)

    iface = SimpleNamespace(device="cpu", flow_norm=0.05, cropAndResize=TartanStereoVOMotion.cropAndResize,
                            pose_norm=torch.tensor([0.13, 0.13, 0.13, 0.013, 0.013, 0.013], dtype=torch.float),
                            model=SimpleNamespace(stereoNormFactor=0.02, poseDepthNormFactor=0.25, flowPoseNet=flow_pose_net))

    def frame_of(H, W):
        return SimpleNamespace(stereo=SimpleNamespace(height=H, width=W, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"],
                                                      frame_baseline=CAM["baseline"]))

    out = {"cam": np.array([CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])}
    for name, H, W, seed, special in CASES:
        flow, depth = inputs(H, W, seed, special)
        captured.clear()
        raw = TartanStereoVOMotion.inference(iface, frame_of(H, W), flow, depth)
        x = captured[0]
        assert x.shape == (1, 5, 112, 160)
        out[f"{name}_sha"] = np.array(sha(x))
        idx = sample_idx(x.numel())
        out[f"{name}_sample"] = x.reshape(-1)[idx].numpy()
        out[f"{name}_raw"] = raw.numpy()

    # TartanMotionNet.predict / update over a sequence (MACVO.py:160,193-194: predict(frame0, None, ...) first, then update + predict)
    mm = object.__new__(MM.TartanMotionNet)
    mm.config = SimpleNamespace(weight="", device="cpu")
    mm.model = SimpleNamespace(inference=lambda frame, flow, depth: TartanStereoVOMotion.inference(iface, frame, flow, depth))
    mm.prev_pose = None
    poses = [mm.predict(frame_of(SEQ_H, SEQ_W), None, None).tensor().reshape(7)]
    for k in range(1, SEQ_FRAMES):
        mm.update(pp.SE3(seq_update(poses[-1], k)))
        flow, depth = seq_inputs(k)
        poses.append(mm.predict(frame_of(SEQ_H, SEQ_W), flow, depth).tensor().reshape(7))
    out["seq_poses"] = torch.stack(poses).numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "motion_model.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
