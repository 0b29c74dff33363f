"""TEST INFRASTRUCTURE: a from-scratch torch restatement of TartanMotionNet around its PoseNet (MAC-VO ``Module/MotionModel.py:90-123``,
``Module/Network/TartanVOStereo/StereoVO_Interface.py:158-194``), op for op, so that it rounds like the reference on whatever device
it runs: on CPU it is checked against tests/golden/motion_model.npz (the reference's own functions), on the GPU the HIP kernels are
checked against it.  PyPose's se3 Exp / SE3 compose come from tests/golden/pypose_shim.py."""
from __future__ import annotations

import torch
import torch.nn.functional as F

STEREO_NORM, POSE_DEPTH_NORM = 0.02, 0.25              # StereoVONet(stereoNormFactor=0.02, poseDepthNormFactor=0.25), StereoVO_Interface.py:28
POSE_NORM = [0.13, 0.13, 0.13, 0.013, 0.013, 0.013]    # :51-53
FLOW_NORM = 0.05                                       # :54


def intrinsic_layer(w, h, fx, fy, ox, oy, device):
    """make_device_intrinsic_layer (TartanVOStereo/Utility.py:13-18): ``ij`` meshgrid over (w, h), stacked (hh, ww)."""
    ww, hh = torch.meshgrid(torch.arange(w, device=device), torch.arange(h, device=device), indexing="ij")
    ww = (ww.float() - ox + 0.5) / fx
    hh = (hh.float() - oy + 0.5) / fy
    return torch.stack((hh, ww), dim=-1)


def center_crop_to(x, shape, dims):
    """Utility/Utils.py:65-72: narrow by (size - target) // 2 on each side (an odd difference keeps one more element)."""
    for s, d in zip(shape, dims):
        size = x.size(d)
        to_crop = (size - s) // 2
        if to_crop != 0:
            x = x.narrow(d, to_crop, size - 2 * to_crop)
    return x


def crop_and_resize(x, target=(112, 160)):
    """TartanStereoVOMotion.cropAndResize (StereoVO_Interface.py:162-174)."""
    th, tw = target
    s = min(int(x.shape[-2] / th), int(x.shape[-1] / tw))
    x = center_crop_to(x, [th * s, tw * s], [-2, -1])
    return F.interpolate(x, size=(th, tw), mode="bilinear", align_corners=True)


def motion_input(flow, depth, fx, fy, cx, cy, baseline):
    """The PoseNet input of TartanStereoVOMotion.inference (:177-188): flow ``[1,2,H,W]``, depth ``[1,1,H,W]`` -> ``[1,5,112,160]``.
    The intrinsic layer is built with the reference's argument order (height, width) -> (w, h)."""
    H, W = flow.shape[-2:]
    intr = intrinsic_layer(H, W, fx, fy, cx, cy, flow.device).unsqueeze(0).permute(0, 3, 1, 2)
    intr = crop_and_resize(intr)
    d = crop_and_resize(depth)
    fl = crop_and_resize(flow) * FLOW_NORM
    stereo = (baseline * fx) / d
    stereo = torch.nan_to_num(stereo * STEREO_NORM, nan=0.0).clamp(min=0.0)
    d = stereo / (baseline * fx) / float(STEREO_NORM * POSE_DEPTH_NORM)
    return torch.cat((fl, d, intr), dim=1)


def compose(prev, raw, pp):
    """``prev @ pp.se3(raw.squeeze() * pose_norm).Exp()`` (MotionModel.py:112, StereoVO_Interface.py:194) in the dtype of ``prev``."""
    m = raw.to(prev.dtype) * torch.tensor(POSE_NORM, dtype=prev.dtype, device=prev.device)     # ([6] or [n, 6]: shapes as given)
    out = pp.SE3(prev) @ pp.LieTensor(m, ltype="se3").Exp()
    return out.tensor() if hasattr(out, "tensor") else out


class MotionModelRef:
    """TartanMotionNet.predict / update (MotionModel.py:102-118) with the PoseNet as a callable ``[1,5,112,160] -> [1,6]``."""

    def __init__(self, pose_net, pp, device):
        self.net, self.pp, self.device = pose_net, pp, device
        self.prev_pose = None

    def predict(self, flow, depth, fx, fy, cx, cy, baseline):
        if self.prev_pose is None:
            self.prev_pose = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=self.device)
            return self.prev_pose.clone()
        raw = self.net(motion_input(flow, depth, fx, fy, cx, cy, baseline))
        self.prev_pose = compose(self.prev_pose, raw.reshape(6).float(), self.pp).reshape(7)
        return self.prev_pose

    def update(self, pose):
        self.prev_pose = pose.to(self.device).reshape(7)
