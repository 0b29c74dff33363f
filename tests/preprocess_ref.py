"""TEST INFRASTRUCTURE: the resampling family of the reference's DataLoader/Transform.py (:41-209) restated on the CPU.

The reference calls torchvision's ``resize`` and ``center_crop`` on tensors; torchvision is not a dependency here and the reference does not pin it, so the
two are restated from torchvision's tensor path — ``resize`` -> ``F.interpolate`` (``nearest-exact`` for ``InterpolationMode.NEAREST_EXACT``, bilinear with
``antialias=True``, the tensor default; non-fp32 planes go through fp32 and are cast back without rounding unless they are integers), ``center_crop`` -> pad
then slice — and everything around them is the reference's own lines.  RESTATED, PARITY-UNPINNED.  The fp64 formula of the antialias filter stands beside
it (``aa_matrix``) for the error measurements."""
from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F


def resize(img: torch.Tensor, size, interp: str) -> torch.Tensor:
    """torchvision.transforms.functional.resize(img, [h, w], interpolation=BILINEAR | NEAREST_EXACT) on a tensor."""
    if list(img.shape[-2:]) == list(size):
        return img
    dt = img.dtype
    x = img if dt in (torch.float32, torch.float64) else img.to(torch.float32)
    if interp == "bilinear":
        y = F.interpolate(x, size=list(size), mode="bilinear", align_corners=False, antialias=True)
    else:
        y = F.interpolate(x, size=list(size), mode="nearest-exact")
    if y.dtype != dt:
        if dt in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            y = torch.round(y)
        y = y.to(dt)
    return y


def center_crop(img: torch.Tensor, size) -> torch.Tensor:
    """torchvision.transforms.functional.center_crop on a tensor: zero-pad an axis that is smaller than the crop, then cut at Python's round()."""
    th, tw = size
    h, w = img.shape[-2:]
    if tw > w or th > h:
        left, top = ((tw - w) // 2 if tw > w else 0), ((th - h) // 2 if th > h else 0)
        right, bottom = ((tw - w + 1) // 2 if tw > w else 0), ((th - h + 1) // 2 if th > h else 0)
        padded = torch.zeros(img.shape[:-2] + (h + top + bottom, w + left + right), dtype=img.dtype)
        padded[..., top:top + h, left:left + w] = img
        img = padded
        h, w = img.shape[-2:]
        if tw == w and th == h:
            return img
    top = int(round((h - th) / 2.0))
    left = int(round((w - tw) / 2.0))
    return img[..., top:top + th, left:left + tw]


def stereo(imageL, imageR, K, gt_flow=None, flow_mask=None, gt_depth=None) -> SimpleNamespace:
    return SimpleNamespace(imageL=imageL, imageR=imageR, gt_flow=gt_flow, flow_mask=flow_mask, gt_depth=gt_depth, K=K,
                           height=int(imageL.shape[-2]), width=int(imageL.shape[-1]))


def scale_stereo(data, scale_u: float, scale_v: float, interpolate: str):
    """Transform.py:54-88."""
    raw_height, raw_width = data.height, data.width
    target_h, target_w = int(raw_height / scale_v), int(raw_width / scale_u)
    round_scale_v, round_scale_u = raw_height / target_h, raw_width / target_w
    data.K = data.K.clone()
    data.height, data.width = target_h, target_w
    data.K[:, 0] /= round_scale_u
    data.K[:, 1] /= round_scale_v
    data.imageL = resize(data.imageL, [target_h, target_w], interpolate)
    data.imageR = resize(data.imageR, [target_h, target_w], interpolate)
    if data.gt_flow is not None:
        data.gt_flow = resize(data.gt_flow, [target_h, target_w], interpolate).clone()
        data.gt_flow[:, 0] /= round_scale_u
        data.gt_flow[:, 1] /= round_scale_v
    if data.flow_mask is not None:
        data.flow_mask = resize(data.flow_mask, [target_h, target_w], interpolate)
    if data.gt_depth is not None:
        data.gt_depth = resize(data.gt_depth, [target_h, target_w], interpolate)
    return data


def crop_stereo(data, target_h: int, target_w: int):
    """Transform.py:109-127."""
    orig_h, orig_w = data.height, data.width
    for n in ("imageL", "imageR", "gt_flow", "flow_mask", "gt_depth"):
        if getattr(data, n) is not None:
            setattr(data, n, center_crop(getattr(data, n), [target_h, target_w]))
    data.K = data.K.clone()
    data.height, data.width = target_h, target_w
    data.K[:, 0, 2] -= (orig_w - target_w) / 2.
    data.K[:, 1, 2] -= (orig_h - target_h) / 2.
    return data


def smart_resize(data, height: int, width: int, interp: str):
    """Transform.py:197-209."""
    scale_factor = min(data.height / height, data.width / width)
    data = scale_stereo(data, scale_factor, scale_factor, interp)
    return crop_stereo(data, height, width)


_CAST = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def cast(data, dtype: str):
    """Transform.py:172-178."""
    for n in ("imageL", "imageR", "gt_flow", "gt_depth", "flow_mask"):
        if getattr(data, n) is not None:
            setattr(data, n, getattr(data, n).to(dtype=_CAST[dtype]))
    return data


def apply(data, steps):
    """``[(kind, args), ...]`` in the vocabulary of ``ops.preprocess_plan`` on a copy of ``data``."""
    data = copy.copy(data)
    for kind, a in steps:
        if kind == "scale":
            data = scale_stereo(data, a["scale_u"], a["scale_v"], a["interp"])
        elif kind == "crop":
            data = crop_stereo(data, a["height"], a["width"])
        elif kind == "smart":
            data = smart_resize(data, a["height"], a["width"], a["interp"])
        else:
            data = cast(data, a["dtype"])
    return data


def smart_geometry(H: int, W: int, th: int, tw: int, K: torch.Tensor):
    """SmartResizeFrame's host arithmetic alone (no planes): resized size, crop origin, pads (top, bottom, left, right), K [1, 3, 3] after it."""
    s = min(H / th, W / tw)
    rh, rw = int(H / s), int(W / s)
    K = K.clone()
    K[:, 0] /= W / rw
    K[:, 1] /= H / rh
    pt, pb = ((th - rh) // 2, (th - rh + 1) // 2) if th > rh else (0, 0)
    pl, pr = ((tw - rw) // 2, (tw - rw + 1) // 2) if tw > rw else (0, 0)
    top, left = int(round((rh + pt + pb - th) / 2.0)), int(round((rw + pl + pr - tw) / 2.0))
    K[:, 0, 2] -= (rw - tw) / 2.
    K[:, 1, 2] -= (rh - th) / 2.
    return (rh, rw), (top, left), (pt, pb, pl, pr), K


# ---- the antialias filter's formula in fp64 (what F.interpolate(mode="bilinear", antialias=True) computes per axis)
def aa_window(i: int, n_in: int, n_out: int):
    if n_in == n_out:
        return i, 1
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    center = scale * (i + 0.5)
    xmin = max(0, int(center - support + 0.5))
    xmax = min(n_in, int(center + support + 0.5))
    return xmin, xmax - xmin


def aa_weights(i: int, n_in: int, n_out: int) -> np.ndarray:
    xmin, xsize = aa_window(i, n_in, n_out)
    if n_in == n_out:
        return np.ones(1)
    scale = n_in / n_out
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    center = scale * (i + 0.5)
    w = np.array([max(0.0, 1.0 - abs((j - center + 0.5) * invscale)) for j in range(xmin, xmin + xsize)])
    w[w <= 1e-12] = 0.0           # a tap at the exact edge of the support: 0 in exact arithmetic, a few 1e-15 of rounding noise in fp64
    return w / w.sum()


def aa_matrix(n_in: int, n_out: int) -> np.ndarray:
    M = np.zeros((n_out, n_in))
    for i in range(n_out):
        xmin, xsize = aa_window(i, n_in, n_out)
        M[i, xmin:xmin + xsize] = aa_weights(i, n_in, n_out)
    return M


def aa_resize_f64(x: torch.Tensor, size) -> torch.Tensor:
    """The formula on ``x`` ``[..., H, W]`` in fp64: width pass, then height pass."""
    Wy = torch.from_numpy(aa_matrix(x.shape[-2], size[0]))
    Wx = torch.from_numpy(aa_matrix(x.shape[-1], size[1]))
    return Wy @ (x.double() @ Wx.T)
