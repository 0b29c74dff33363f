"""Stereo rectification of a calibrated rig — what ``EuRoC_StereoSequence`` and ``VBR_StereoSequence`` do with OpenCV on the host (DataLoader/Dataset/EuRoC.py:
143-174, 231-236; VBR.py:60-64, 155-180) — as one host plan, one map launch per sequence and ONE remap launch per frame (``ops.stereo_rectify_plan``,
``ops.rectify_maps``, ``ops.remap``).  OpenCV is restated, parity-unpinned (``include/macvo_hip.h``).  Reading image files, matching the two cameras' time
stamps and loading ground-truth poses stay with the caller."""
from __future__ import annotations

import torch

from . import ops


class StereoRectifier:
    """``StereoRectifier(K1, D1, K2, D2, size, R, T, device)``: the plan (``cv2.stereoRectify`` with ``CALIB_ZERO_DISPARITY``, ``alpha = -1``) and both
    cameras' maps (``cv2.initUndistortRectifyMap``, ``CV_32FC1``), built once.  ``size`` = ``(width, height)``; ``R``, ``T`` take camera 1 (left) to camera 2.

    ``K`` is the rectified ``P1[:3, :3]`` as ``[1, 3, 3]`` fp32 — the ``K`` of ``EuRoC_StereoSequence`` that back-projection, the PGO and
    ``ops.preprocess_plan`` take; ``baseline`` = ``|P2[idx][3] / fc|``.  Calling the object remaps a left and a right uint8 image batch in one launch."""

    def __init__(self, K1, D1, K2, D2, size, R, T, device="cuda"):
        self.plan = ops.stereo_rectify_plan(K1, D1, K2, D2, size, R, T)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.width, self.height = int(size[0]), int(size[1])
        self.map_x, self.map_y = ops.rectify_maps(self.plan, device=self.device)          # [2, H, W] each: left, right
        self.K = self.plan.K.unsqueeze(0)
        self.baseline = self.plan.baseline
        self.R1, self.R2, self.P1, self.P2 = self.plan.R1, self.plan.R2, self.plan.P1, self.plan.P2

    @classmethod
    def from_body_frames(cls, T_BS_l, intr_l, D_l, T_BS_r, intr_r, D_r, size, device="cuda") -> "StereoRectifier":
        """From each camera's sensor-to-body transform (4 x 4) and ``[fx, fy, cx, cy]`` as a ``sensor.yaml`` holds them: ``T_LR = inv(T_BS_r) @ T_BS_l``, as
        both datasets' ``sync_LR`` computes it (EuRoC.py:146, VBR.py:157)."""
        Tl = torch.as_tensor(T_BS_l, dtype=torch.float64).reshape(4, 4)
        Tr = torch.as_tensor(T_BS_r, dtype=torch.float64).reshape(4, 4)
        T_LR = torch.linalg.inv(Tr) @ Tl

        def K_of(i):
            fx, fy, cx, cy = (float(v) for v in i)
            return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)

        return cls(K_of(intr_l), D_l, K_of(intr_r), D_r, size, T_LR[:3, :3], T_LR[:3, 3], device)

    @property
    def maps(self) -> tuple:
        """``((map_x, map_y) of the left camera, (map_x, map_y) of the right camera)``, fp32 ``[H, W]`` device tensors (cv2's CV_32FC1 pairs)."""
        return (self.map_x[0], self.map_y[0]), (self.map_x[1], self.map_y[1])

    def __call__(self, imageL_u8: torch.Tensor, imageR_u8: torch.Tensor, dtype=torch.float32, layout: str = "hwc", reverse_channels: bool = False,
                 out: "list | None" = None) -> tuple:
        """Both images of every lane through their camera's map in ONE launch on the current stream -> ``(imageL, imageR)``, each ``[lanes, C, H, W]``:
        what ``EurocMonocularDataset.__getitem__`` yields per camera (``dtype=torch.float32``: remapped / 255), or planar uint8 (``dtype=torch.uint8``),
        which ``ops.preprocess`` takes as it is at a quarter of the traffic.  ``layout="hwc"``: ``[lanes, H, W, C]`` as ``cv2.imread`` returns them;
        ``reverse_channels=True`` is VBR's BGR -> RGB."""
        l, r = ops.remap([imageL_u8, imageR_u8], list(self.maps), dtype=dtype, layout=layout, reverse_channels=reverse_channels, out=out)
        return l, r
