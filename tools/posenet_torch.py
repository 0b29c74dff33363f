"""The TartanVO PoseNet in plain torch: a restatement of ``VOFlowRes(config=1, stereo=True, down_scale=True, intrinsic=True)``
(MAC-VO ``Module/Network/TartanVOStereo/FlowPoseNet.py:45-166`` as ``StereoVO.py:21`` builds it), loadable from the same state dict.

It is the reference of the HIP forward's tests (``ops.PoseNet``) and the eager baseline of ``tools/motion_model_run.py --pose-net torch``.
``seeded_state_dict`` makes weights whose signal neither vanishes nor explodes through the 46 layers (torch's default initialisation
vanishes), so a test compares O(10) outputs, not noise.
"""
from __future__ import annotations

import hashlib
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

BLOCKS = (3, 4, 6, 7, 3)            # BasicBlocks of layer1..layer5
PLANES = (64, 128, 128, 256, 256)
STAGES = ("firstconv", "layer1", "layer2", "layer3", "layer4", "layer5")
STAGE_SHAPES = ((32, 56, 80), (64, 28, 40), (128, 14, 20), (128, 7, 10), (256, 4, 5), (256, 2, 3))
IN_SHAPE = (5, 112, 160)
N_PARAMS = 15135430


def _conv_relu(cin: int, cout: int, stride: int) -> nn.Sequential:
    return nn.Sequential(nn.Conv2d(cin, cout, 3, stride, 1), nn.ReLU())


def _linear_relu(cin: int, cout: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(cin, cout), nn.ReLU())


class BasicBlock(nn.Module):
    """conv1 3x3 (stride s) + ReLU, conv2 3x3, + identity (a 1x1 stride-2 conv in a layer's first block), ReLU."""

    def __init__(self, cin: int, planes: int, stride: int, downsample: "nn.Module | None"):
        super().__init__()
        self.conv1 = _conv_relu(cin, planes, stride)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class PoseNetTorch(nn.Module):
    """``forward(x [n,5,112,160]) -> [n,6]`` = cat(trans, rot), the raw motion before ``pose_norm``; ``return_stages=True`` also returns
    the outputs of firstconv and layer1..5."""

    def __init__(self):
        super().__init__()
        self.firstconv = nn.Sequential(_conv_relu(IN_SHAPE[0], 32, 2), _conv_relu(32, 32, 1), _conv_relu(32, 32, 1))
        cin = 32
        for i, (n, planes) in enumerate(zip(BLOCKS, PLANES)):
            blocks = [BasicBlock(cin, planes, 2, nn.Conv2d(cin, planes, 1, 2))]
            blocks += [BasicBlock(planes, planes, 1, None) for _ in range(n - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = planes
        for name in ("voflow_trans", "voflow_rot"):
            setattr(self, name, nn.Sequential(_linear_relu(cin * 6, 128), _linear_relu(128, 32), nn.Linear(32, 3)))

    def forward(self, x, return_stages: bool = False):
        stages = []
        for name in STAGES:
            x = getattr(self, name)(x)
            stages.append(x)
        f = x.reshape(x.shape[0], -1)
        y = torch.cat((self.voflow_trans(f), self.voflow_rot(f)), dim=1)
        return (y, stages) if return_stages else y


def tensor_table() -> "list[tuple[str, tuple[int, ...]]]":
    """(key, shape) of the 120 tensors in ``state_dict()`` order."""
    with torch.device("meta"):
        net = PoseNetTorch()
    return [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def seeded_state_dict(seed: int) -> "dict[str, torch.Tensor]":
    """One generator walks the canonical tensor order: 4-D ``randn * sqrt(2 / fan_in)`` (``*.conv2.weight`` halved, so a residual sum
    keeps its scale), 2-D ``randn * sqrt(2 / in_features)``, 1-D ``randn * 0.1``."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in tensor_table():
        t = torch.randn(shape, generator=g, dtype=torch.float32)
        if len(shape) == 4:
            t = t * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
            if key.endswith(".conv2.weight"):
                t = t * 0.5
        elif len(shape) == 2:
            t = t * math.sqrt(2.0 / shape[1])
        else:
            t = t * 0.1
        sd[key] = t
    return sd


def state_dict_sha256(sd: "dict[str, torch.Tensor]") -> str:
    h = hashlib.sha256()
    for key, t in sd.items():
        h.update(key.encode())
        h.update(t.detach().to("cpu", torch.float32).contiguous().numpy().tobytes())
    return h.hexdigest()


def sample_input(lanes: int = 3, seed: int = 5) -> torch.Tensor:
    """``randn(lanes,5,112,160)`` with the depth channel made positive (``|.| * 3``)."""
    x = torch.randn((lanes,) + IN_SHAPE, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    x[:, 2] = x[:, 2].abs() * 3
    return x


def from_state_dict(sd, device="cpu", dtype=torch.float32) -> PoseNetTorch:
    net = PoseNetTorch()
    net.load_state_dict({k: v for k, v in sd.items()}, strict=True)
    return net.to(device=device, dtype=dtype).eval()


def sample_index(numel: int, n: int = 512) -> torch.Tensor:
    """``n`` evenly spread flat indices of a tensor (the golden stores the stage outputs at these)."""
    return torch.linspace(0, numel - 1, n, dtype=torch.float64).round().long()
