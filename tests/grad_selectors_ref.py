"""Torch restatements of the reference's image-gradient keypoint selectors and of SelectorCompose (Module/KeypointSelector.py:121-158 GradientSelector,
:161-213 SparseGradienSelector, :51-75 SelectorCompose) on CPU ops, for the tests: pinned against the reference's own classes by
tests/golden/grad_selectors.npz, used where the reference tree is absent.  The draw takes a ``generator`` (None: torch's global CPU generator)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

LAPLACIAN = ((0, 1, 0), (1, -4, 1), (0, 1, 0))


def image_grad(image: torch.Tensor) -> torch.Tensor:
    """``[3, H, W]`` fp32 -> ``[1, H, W]``: |conv2d with the Laplacian expanded over the three channels, padding 1| (:129-135)."""
    return F.conv2d(image.unsqueeze(0), torch.tensor(LAPLACIAN).float().expand((1, 3, 3, 3)), padding=1)[0].abs()


def threshold(grad: torch.Tensor, grad_std: float) -> torch.Tensor:
    return grad.mean(dim=(1, 2), keepdim=True) + grad_std * grad.std(dim=(1, 2), keepdim=True)


def candidate_mask(image: torch.Tensor, mask_width: int, grad_std: float, nms_size: "int | None" = None) -> torch.Tensor:
    """bool ``[1, H, W]``: the pixels ``torch.nonzero`` lists (:139-147, :182-201)."""
    grad = image_grad(image.float().cpu())
    points = grad > threshold(grad, grad_std)
    border = torch.zeros_like(points)
    border[..., mask_width:-mask_width, mask_width:-mask_width] = 1.0      # (0:-0 is the empty slice)
    points = points * border
    if nms_size is not None:
        points = points * (grad == F.max_pool2d(grad, kernel_size=nms_size, stride=1, padding=nms_size // 2))
    return points


def candidates(image: torch.Tensor, mask_width: int, grad_std: float, nms_size: "int | None" = None) -> torch.Tensor:
    """int64 ``[n]`` row-major linear indices ``v * W + u``."""
    vu = torch.nonzero(candidate_mask(image, mask_width, grad_std, nms_size), as_tuple=False)[:, 1:]
    return vu[:, 0] * image.shape[-1] + vu[:, 1]


def select(image: torch.Tensor, num_point: int, mask_width: int, grad_std: float, nms_size: "int | None" = None,
           generator: "torch.Generator | None" = None) -> torch.Tensor:
    """``select_point``: int64 ``[min(n, num_point), 2]`` (u, v) (:147-151, :201-205)."""
    selected = torch.nonzero(candidate_mask(image, mask_width, grad_std, nms_size), as_tuple=False)
    n = selected.shape[0]
    perm = (torch.randperm(n) if generator is None else torch.randperm(n, generator=generator))[:num_point]
    return selected[perm][..., 1:].roll(shifts=1, dims=1)


def compose_split(weight, num_point: int) -> list:
    """What SelectorCompose asks of each sub-selector (:60-61, :66): fp32 weights normalised in fp32, an fp32 product, truncated."""
    w = torch.tensor(weight)
    w = w / w.sum()
    return [int(num_point * wi) for wi in w]


def compose(selects, weight, num_point: int) -> torch.Tensor:
    """``selects``: one callable ``num_point -> rows`` per sub-selector; the rows concatenated in order (:63-67)."""
    return torch.cat([s(k) for s, k in zip(selects, compose_split(weight, num_point))], dim=0)


# ---- the suite's inputs --------------------------------------------------------------------------------------------------------------------------------
def quantised_u8(H: int, W: int, seed: int) -> np.ndarray:
    """uint8 ``[3, H, W]``: a smoothed random field with texture, so that the gradient has structure, ties and flat spots."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(3, H, W)).astype(np.float64)
    smooth = base.copy()
    for _ in range(2):
        smooth = (smooth + np.roll(smooth, 1, 1) + np.roll(smooth, -1, 1) + np.roll(smooth, 1, 2) + np.roll(smooth, -1, 2)) / 5.0
    mix = np.where(rng.random((1, H, W)) < 0.15, base, smooth)
    return np.clip(np.rint(mix), 0, 255).astype(np.uint8)


def quantised_image(H: int, W: int, seed: int, denom: int = 256) -> torch.Tensor:
    """``[3, H, W]`` fp32 with values ``k / denom``.  denom 256: every step of the selectors is exact in fp32; 255: general floats."""
    return torch.from_numpy(quantised_u8(H, W, seed).astype(np.float32)) / float(denom)


def block_constant_image(H: int, W: int, seed: int, block: int = 4) -> torch.Tensor:
    """1/256-valued image constant over ``block x block`` cells: the gradient has exact ties inside every NMS window."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(3, (H + block - 1) // block, (W + block - 1) // block)).astype(np.uint8)
    k = np.repeat(np.repeat(k, block, 1), block, 2)[:, :H, :W]
    return torch.from_numpy(k.astype(np.float32)) / 256.0


def threshold_f64(image: torch.Tensor, grad_std: float):
    """(grad fp64 [H, W], thr fp64) of an fp64 evaluation."""
    g = F.conv2d(image.double().unsqueeze(0), torch.tensor(LAPLACIAN).double().expand((1, 3, 3, 3)), padding=1)[0, 0].abs()
    return g, float(g.mean() + float(grad_std) * g.std())


def guard_distance(image: torch.Tensor, grad_std: float, denom: int = 256) -> float:
    """Distance of the fp64 threshold from the nearest multiple of 1 / denom (the values the gradient of a 1 / denom-valued image takes)."""
    _, thr = threshold_f64(image, grad_std)
    return abs(thr * denom - round(thr * denom)) / denom


# the golden file's cases: (H, W, image seed, mask_width, grad_std, nms_size or None, num_point, torch.manual_seed)
GOLDEN_CASES = ((96, 128, 3, 8, 1.0, None, 200, 11), (96, 128, 3, 8, 2.0, 7, 200, 12), (61, 83, 5, 4, 1.0, 3, 50, 13), (61, 83, 5, 4, 3.0, None, 500, 14),
                (33, 200, 7, 2, 2.0, 15, 64, 15), (33, 200, 7, 0, 1.0, 3, 64, 16))
# SelectorCompose: GradientSelector + SparseGradienSelector on GOLDEN_CASES[0]'s image, weights [1, 3], numPoint 101 under manual_seed 21
GOLDEN_COMPOSE = dict(H=96, W=128, image_seed=3, mask_width=8, grad_std=1.0, nms_size=5, weight=[1, 3], num_point=101, seed=21)
