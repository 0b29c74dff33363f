"""Torch restatements of the reference's map-less keypoint selectors (Module/KeypointSelector.py:103-118 RandomSelector, :216-247 GridSelector) for the
tests: pinned against the reference's own classes by tests/golden/selectors.npz (tests/test_selectors_host.py), used where the reference tree is absent."""
from __future__ import annotations

import math

import torch


def random_select(num_point: int, H: int, W: int, mask_width: int, generator: "torch.Generator | None" = None) -> torch.Tensor:
    """int64 [num_point, 2] (u, v): the rows' v are drawn first, then their u; duplicates are kept."""
    kw = {} if generator is None else {"generator": generator}
    h = torch.randint(mask_width, H - mask_width, (num_point, 1), **kw)
    w = torch.randint(mask_width, W - mask_width, (num_point, 1), **kw)
    return torch.cat([w, h], dim=1)


def grid_select(num_point: int, H: int, W: int, mask_width: int) -> torch.Tensor:
    """int64 [rows, 2] (u, v); rows follows from the shape and may exceed num_point.  Raises (ZeroDivisionError / RuntimeError) where the
    reference does."""
    h, w = H - 2 * mask_width, W - 2 * mask_width
    unit = max(1, int(math.sqrt(num_point // 2)))
    mesh_u, mesh_v = torch.meshgrid(torch.arange(0, h, h // unit), torch.arange(0, w, w // (unit * 2)), indexing="ij")
    return torch.stack([mesh_v.flatten(), mesh_u.flatten()], dim=1) + mask_width


def grid_count(num_point: int, H: int, W: int, mask_width: int) -> int:
    """Row count of grid_select; 0 where it raises or the masked image is empty."""
    try:
        if H <= 2 * mask_width or W <= 2 * mask_width:
            return 0
        return int(grid_select(num_point, H, W, mask_width).shape[0])
    except (ZeroDivisionError, RuntimeError):
        return 0


# (H, W, mask_width, numPoint) of the golden file — 640x480/32/200 and 1280x720 give 231 grid rows, 2000 gives 2048, mask 0 exactly 200
CASES = ((480, 640, 32, 200), (720, 1280, 32, 200), (480, 640, 32, 2000), (480, 640, 0, 200), (480, 640, 32, 1), (96, 128, 5, 50), (192, 256, 16, 512),
         (480, 640, 32, 512))
RANDOM_SEEDS = (5, 1234)
RANDOM_CALLS = 8          # successive select_point calls of one generator, followed by one torch.randperm(RANDPERM_N)[:RANDPERM_K]
RANDPERM_N, RANDPERM_K = 7000, 200
# shapes where the reference's GridSelector raises (a step of 0)
GRID_RAISES = ((64, 640, 30, 200), (480, 56, 20, 200), (480, 640, 236, 200))
