"""TEST INFRASTRUCTURE: the maps and images the remap tests share (tests/test_rectify_host.py pins the host twin to the numpy formula on them,
tests/test_gpu_rectify.py the kernel to the twin)."""
from __future__ import annotations

import numpy as np

SRC_HW, OUT_HW, LANES = (37, 53), (29, 61), 3      # the output size differs from the source; 61 is no multiple of any vector width


def crafted_values(size: int) -> np.ndarray:
    """Map coordinates along an axis of ``size`` source pixels where the fixed-point arithmetic can go wrong."""
    ties = [(k + 0.5) / 32 for k in (4, 5, 320, 321, -2, -3, -1, 0)]                  # map * 32 exactly k + 0.5, k even and odd: half to EVEN
    neg = [-0.25, -0.5, -0.99, -1.0 / 32, -31.0 / 32, -1e-6]                           # inside (-1, 0): floor and truncation differ
    edge = [size - 1 + 0.5, size - 1.0, size - 1 + 1.0 / 32, size - 0.5 / 32, float(size), 0.0, -1.0, -1.0 - 1.0 / 32]
    far = [1e9, -1e9, np.inf, -np.inf, np.nan, 2.0 ** 25, -2.0 ** 25, 2.0 ** 25 + 4, -2.0 ** 25 - 4, 3.0e38]   # 2^25 * 32 = 2^30: the last value kept
    return np.array(ties + neg + edge + far, np.float32)


def crafted_maps(src_hw=SRC_HW, out_hw=OUT_HW, seed: int = 0, lanes: int | None = None):
    """fp32 (map_x, map_y) ``[h, w]`` (or ``[lanes, h, w]``): random within [-3, size + 3], the first entries every crafted x against every crafted y."""
    rng = np.random.default_rng(seed)
    H, W = src_hw
    shape = out_hw if lanes is None else (lanes,) + tuple(out_hw)
    mx = rng.uniform(-3, W + 3, shape).astype(np.float32)
    my = rng.uniform(-3, H + 3, shape).astype(np.float32)
    cx, cy = crafted_values(W), crafted_values(H)
    gx, gy = np.meshgrid(cx, cy, indexing="ij")
    n = gx.size
    assert n <= out_hw[0] * out_hw[1]
    for m, g in ((mx, gx), (my, gy)):
        flat = m.reshape(-1, out_hw[0] * out_hw[1])
        flat[:, :n] = g.reshape(-1)
        # a few random entries quantised to 1/64: more ties, inside and on the border
        pick = rng.integers(n, flat.shape[1], 200)
        flat[:, pick] = np.round(flat[:, pick] * 64) / 64
    return mx, my


def images(channels: int, layout: str, src_hw=SRC_HW, lanes: int = LANES, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed + channels)
    H, W = src_hw
    shape = (lanes, H, W, channels) if layout == "hwc" else (lanes, channels, H, W)
    return rng.integers(0, 256, shape, dtype=np.uint8)
