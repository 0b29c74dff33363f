"""CPU restatement of the reference's four per-frame evaluations (Evaluation/EvalFlow.py:29-47,82-127, Evaluation/EvalDepth.py:22-34,57-82,
Utility/Extensions/GridRecorder.py:24-36) in the fp32 closed form that ``include/macvo_hip.h`` documents, op for op (one torch op per rounding),
with fp64 means of the same fp32 per-pixel terms.  ``tests/test_eval_host.py`` pins it to the reference's own functions (tests/golden/eval.npz);
the GPU tests compare the kernels with it.

A frame is ``est [2,H,W]`` / ``[H,W]`` etc.; every function returns a dict keyed by the row's column names (``_lib.EVAL_*_COLS``), plus the
per-pixel planes and grids."""
from __future__ import annotations

import math

import numpy as np
import torch

NAN = float("nan")
GRID = 100


# ------------------------------------------------------------------------------------------------ building blocks
def quantile(values: torch.Tensor, q: float) -> float:
    """torch.nanquantile's rule on fp32 (linear interpolation): n non-NaN values, r = fp32(q) * fp32(n - 1), a = v[floor r], b = v[ceil r],
    w = r - floor r, d = b - a, w < 0.5 ? a + w * d : b - d * (1 - w).  NaN for an empty / all-NaN population."""
    v = values.flatten().float()
    v = torch.sort(v[~torch.isnan(v)]).values.numpy()
    n = v.shape[0]
    if n == 0:
        return NAN
    with np.errstate(all="ignore"):
        r = np.float32(q) * np.float32(n - 1)
        fl = np.floor(r)
        a, b = v[int(fl)], v[int(np.ceil(r))]
        w = np.float32(r - fl)
        d = np.float32(b - a)
        res = np.float32(a + np.float32(w * d)) if w < np.float32(0.5) else np.float32(b - np.float32(d * np.float32(np.float32(1) - w)))
    return float(res)


def lower_median(values: torch.Tensor) -> float:
    """torch.nanmedian: the lower middle element of the non-NaN values."""
    v = values.flatten().float()
    v = torch.sort(v[~torch.isnan(v)]).values
    return float(v[(v.numel() - 1) // 2]) if v.numel() else NAN


def pinv_diag2(cu: torch.Tensor, cv: torch.Tensor):
    """Tensor.pinverse of diag(cu, cv): 1 / c where |c| > 1e-15 * max(|cu|, |cv|), else 0 (rcond = 1e-15)."""
    cut = torch.maximum(cu.abs(), cv.abs()) * 1e-15
    cut = torch.where(torch.isnan(cu.abs()), cv.abs() * 1e-15, torch.where(torch.isnan(cv.abs()), cu.abs() * 1e-15, cut))   # fmaxf drops a NaN operand
    zero = torch.zeros_like(cu)
    return torch.where(cu.abs() > cut, 1.0 / cu, zero), torch.where(cv.abs() > cut, 1.0 / cv, zero)


def pinv_1(c: torch.Tensor) -> torch.Tensor:
    """Tensor.pinverse of a 1 x 1: c != 0 ? 1 / c : 0."""
    return torch.where(c != 0, 1.0 / c, torch.zeros_like(c))


def grid_store(grid: np.ndarray, axis0: torch.Tensor, axis1: torch.Tensor, scale: float) -> None:
    """GridRecorder.store with start 0: index = (v * scale).astype(int), counted when both are in [0, 100); accumulates."""
    with np.errstate(all="ignore"):
        i0 = (axis0.numpy().astype(np.float32) * np.float32(scale)).astype(int)
        i1 = (axis1.numpy().astype(np.float32) * np.float32(scale)).astype(int)
    m = (0 <= i0) & (i0 < GRID) & (0 <= i1) & (i1 < GRID)
    np.add.at(grid, (i0[m], i1[m]), 1)


def nanmean64(terms: torch.Tensor):
    """(fp64 mean of the non-NaN fp32 terms, their count)."""
    t = terms.flatten().double()
    keep = ~torch.isnan(t)
    c = int(keep.sum())
    return (float(t[keep].sum() / c) if c else NAN), c


def nanmean32(terms: torch.Tensor) -> float:
    """The reference's own reduction: torch's fp32 ``nanmean().item()`` (what tests/golden/eval.npz holds; the kernels and the fp64 means above
    are within fp32 summation error of it)."""
    return float(terms.flatten().float().nanmean())


# ------------------------------------------------------------------------------------------------ per-pixel terms
def _sqrt(t: torch.Tensor, mode: str) -> torch.Tensor:
    """"ieee": the correctly rounded square root (numpy's; what sqrtf is on the device and torch.sqrt is on a GPU).  "torch": this build's
    torch-CPU sqrt, which on contiguous fp32 tensors goes through a vector maths library that is NOT correctly rounded (about 0.5 % of the
    values are 1 ulp off): only for comparing with records that the reference produced with torch on the CPU (tests/golden/eval.npz)."""
    if mode == "torch":
        return t.sqrt()
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.sqrt(t.numpy()))


def flow_pixels(est: torch.Tensor, gt: torch.Tensor, cov: torch.Tensor | None, dtype=torch.float32, sqrt: str = "ieee"):
    """-> epe, eu, ev, nll, uncertainty (nll / uncertainty None without a covariance).  dtype=float64: the same closed form in fp64."""
    est, gt = est.to(dtype), gt.to(dtype)
    eu, ev = est[0] - gt[0], est[1] - gt[1]
    eu2, ev2 = eu * eu, ev * ev
    epe = _sqrt(eu2 + ev2, sqrt)
    if cov is None:
        return epe, eu, ev, None, None
    cu, cv = cov[0].to(dtype), cov[1].to(dtype)
    det = cu * cv
    pu, pv = pinv_diag2(cu, cv)
    m = (eu * pu) * eu + (ev * pv) * ev
    r = _sqrt(m, sqrt)
    return epe, eu, ev, det.log() + r * r, det


def depth_pixels(est: torch.Tensor, gt: torch.Tensor, cov: torch.Tensor | None, dtype=torch.float32, sqrt: str = "ieee"):
    est, gt = est.to(dtype), gt.to(dtype)
    e = est - gt
    if cov is None:
        return e.abs(), e, None, None
    c = cov.to(dtype)
    r = _sqrt((e * pinv_1(c)) * e, sqrt)
    return e.abs(), e, c.log() + r * r, c


# ------------------------------------------------------------------------------------------------ frames
def _cov_fields(out: dict, nll, unc, mask):
    if nll is None:
        out.update(masked_nll=NAN, n_mask_nll=0)
        for q in ("25", "50", "75"):
            out.update({f"q{q}_nll": NAN, f"t{q}": NAN, f"n_q{q}": 0})
        return
    out["masked_nll"], out["n_mask_nll"] = nanmean64(nll[mask])
    out["masked_nll_f32"] = nanmean32(nll[mask])
    for q, name in ((0.25, "25"), (0.5, "50"), (0.75, "75")):
        t = quantile(unc, q)
        qm = unc < t                                            # strict; NaN compares false; the mask is not intersected
        out[f"t{name}"] = t
        out[f"q{name}_nll"], _ = nanmean64(nll[qm])
        out[f"q{name}_nll_f32"] = nanmean32(nll[qm])
        out[f"n_q{name}"] = int(qm.sum())


def flow_frame(est, gt, cov=None, valid=None, max_flow: float = 128.0, apply_max_flow: bool = True, grids: np.ndarray | None = None,
               sqrt: str = "ieee") -> dict:
    """est, gt [2,H,W]; cov [>=2,H,W] or None; valid bool / u8 [H,W] or None.  grids: uint32 [2,100,100], accumulated in place."""
    est, gt = est.float(), gt.float()
    epe, eu, ev, nll, unc = flow_pixels(est, gt, None if cov is None else cov.float(), sqrt=sqrt)
    mask = torch.ones_like(epe, dtype=torch.bool)
    if apply_max_flow:
        mf = torch.tensor(max_flow, dtype=torch.float32)
        mask &= (est[0] < mf) & (est[1] < mf)
    if valid is not None:
        mask &= valid.reshape(epe.shape) != 0
    out = {"epe_px": epe, "nll_px": nll, "unc_px": unc, "mask_px": mask}
    me = epe[mask]
    out["masked_epe"], out["n_mask_finite"] = nanmean64(me)
    out["epe"], out["n_finite"] = nanmean64(epe)
    out["masked_epe_f32"], out["epe_f32"] = nanmean32(me), nanmean32(epe)
    out["n_mask"] = int(mask.sum())
    nm = np.float32(out["n_mask"])
    with np.errstate(all="ignore"):
        for k in (1, 3, 5):
            out[f"px{k}"] = float(np.float32(int((me < k).sum())) / nm)     # (epe[mask] < k).float().mean(): a NaN epe is a miss
    _cov_fields(out, nll, unc, mask)
    if cov is not None and grids is not None:
        grid_store(grids[0], eu * eu, cov[0].float(), 4.0)
        grid_store(grids[1], ev * ev, cov[1].float(), 4.0)
    return out


def depth_frame(est, gt, cov=None, max_depth: float = 80.0, grid: np.ndarray | None = None, sqrt: str = "ieee") -> dict:
    """est, gt, cov [H,W]; grid: uint32 [100,100], accumulated in place."""
    est, gt = est.float(), gt.float()
    err, e, nll, unc = depth_pixels(est, gt, None if cov is None else cov.float(), sqrt=sqrt)
    mask = est < torch.tensor(max_depth, dtype=torch.float32)
    out = {"err_px": err, "nll_px": nll, "unc_px": unc, "mask_px": mask}
    me = err[mask]
    out["masked_err"], out["n_mask_finite"] = nanmean64(me)
    _, out["n_finite"] = nanmean64(err)
    out["masked_err_f32"] = nanmean32(me)
    out["n_mask"] = int(mask.sum())
    out["err_25"], out["err_50"], out["err_75"] = quantile(me, 0.25), lower_median(me), quantile(me, 0.75)
    _cov_fields(out, nll, unc, mask)
    if cov is not None and grid is not None:
        grid_store(grid, e * e, cov.float(), 2.0)
    return out


def nll_means64(kind: str, est, gt, cov, frame: dict) -> dict:
    """The four NLL means with the per-pixel nll evaluated in fp64 (same closed form, same fp32 masks and thresholds): the distance of the fp32
    route from it is the scale of the NLL-mean tolerances."""
    nll = (flow_pixels(est, gt, cov, torch.float64)[3] if kind == "flow" else depth_pixels(est, gt, cov, torch.float64)[2])
    unc = frame["unc_px"]
    out = {"masked_nll": nanmean64(nll[frame["mask_px"]])[0]}
    for name in ("25", "50", "75"):
        out[f"q{name}_nll"] = nanmean64(nll[unc < frame[f"t{name}"]])[0]
    return out


# ------------------------------------------------------------------------------------------------ sequence reducers (Utility/Datatypes.py)
def seq_mean(values):
    values = list(values)
    return sum(values) / len(values)


def seq_median(values):
    s = sorted(values)
    n = len(s)
    return float(s[n // 2]) if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def isclose_nan(a: float, b: float, tol: float = 0.0) -> bool:
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= tol


def nll_scale(kind: str, est, gt, cov) -> torch.Tensor:
    """max(|log det|, m) per pixel in fp32: the magnitude whose ulp bounds the distance between two logf implementations in the nll."""
    est, gt, cov = est.float(), gt.float(), cov.float()
    if kind == "flow":
        eu, ev = est[0] - gt[0], est[1] - gt[1]
        pu, pv = pinv_diag2(cov[0], cov[1])
        r = _sqrt((eu * pu) * eu + (ev * pv) * ev, "ieee")
        return torch.maximum((cov[0] * cov[1]).log().abs(), r * r)
    e = est - gt
    r = _sqrt((e * pinv_1(cov)) * e, "ieee")
    return torch.maximum(cov.log().abs(), r * r)
