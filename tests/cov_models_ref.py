"""Torch restatement of the reference's other observation-covariance models (Module/Covariance/Project2to3.py:48-57,194-323 and
Utility/Math.py:43-93), quirks included: the transposed kernel, the 1e-3 weight threshold, the mixture variance's /2, no
min_depth_cov clamp in the mixture model, no flow_cov clamp under NoCovariance, cov /= det(cov).  CPU tensors; the test oracle of
tests/golden/cov_models.npz."""
from __future__ import annotations

import torch


def gaussian_kernels(cov: torch.Tensor, k: int) -> torch.Tensor:
    """gaussain_full_kernels (Math.py:43-63): [N,2,2] -> normalised [N,k,k] weights."""
    n = cov.shape[0]
    det = cov.det()
    inv = cov.pinverse().float()
    x = torch.linspace(-(k - 1) / 2.0, (k - 1) / 2.0, k)
    idx = torch.stack(torch.meshgrid(x, x, indexing="ij"), dim=-1).unsqueeze(0).repeat(n, 1, 1, 1)
    z = torch.einsum("bxyi,bij,bxyj->bxy", idx, -0.5 * inv, idx).exp()
    ker = z / (2 * torch.pi * torch.sqrt(det)).view(n, 1, 1)
    return ker / ker.sum(dim=[-1, -2], keepdim=True)


def cov_2to3_full(suu, suv, svv, sdd, u, v, d, fx, fy, cx, cy) -> torch.Tensor:
    sxx = (((u - cx).square() * sdd) + (d.square() * suu) + (suu * sdd)) / (fx ** 2)
    syy = (((v - cy).square() * sdd) + (d.square() * svv) + (svv * sdd)) / (fy ** 2)
    sxy = (((u - cx) * (v - cy) * sdd) + (d.square() + sdd) * suv) / (fx * fy)
    sxz = (sdd * (u - cx)) / fx
    syz = (sdd * (v - cy)) / fy
    rows = [[sdd, sxz, syz], [sxz, sxx, sxy], [syz, sxy, syy]]
    return torch.stack([torch.stack(r, dim=-1) for r in rows], dim=-2).double()


def gmm_covariance(kp, depth, depth_cov_map, depth_cov, flow_cov, fx, fy, cx, cy, kernel_size=31, match_cov_default=0.25,
                   min_flow_cov=0.25, return_weights=False):
    n, h = kp.shape[0], kernel_size // 2
    has_flow = flow_cov is not None
    if has_flow:
        flow_cov[..., :2].clamp_(min=min_flow_cov ** 2)
    else:
        flow_cov = torch.ones(n, 3) * match_cov_default
        flow_cov[..., 2] = 0.0
    suu, svv, suv = flow_cov[:, 0], flow_cov[:, 1], flow_cov[:, 2]
    kl = kp.long()
    off = torch.arange(-h, h + 1)
    uu, vv = torch.meshgrid(off, off, indexing="ij")
    au, av = kl[:, 0:1] + uu.reshape(1, -1), kl[:, 1:2] + vv.reshape(1, -1)
    cov2 = torch.stack([torch.stack([suu, suv], -1), torch.stack([suv, svv], -1)], -2)
    w = gaussian_kernels(cov2, kernel_size).flatten(1)
    z = depth[..., av, au].view(n, kernel_size, kernel_size).permute(0, 2, 1).flatten(1)
    c = depth_cov_map[..., av, au].view(n, kernel_size, kernel_size).permute(0, 2, 1).flatten(1)
    p = w.clone()
    p[p < 1e-3] = 0.0
    p = p / p.sum(dim=1, keepdim=True)
    mean = (z * p).sum(dim=1)
    var = (((c + z.square()) * p).sum(dim=1) - mean.square()) / 2
    if (not has_flow) and depth_cov is not None:
        var = depth_cov
    out = cov_2to3_full(suu, suv, svv, var, kp[:, 0].float(), kp[:, 1].float(), mean, fx, fy, cx, cy)
    return (out, w) if return_weights else out


def no_covariance(n: int) -> torch.Tensor:
    return torch.eye(3).unsqueeze(0).repeat(n, 1, 1).double()


def diagonalize(covs: torch.Tensor) -> torch.Tensor:
    covs = covs.clone()
    for i in range(3):
        for j in range(3):
            if i != j:
                covs[..., i, j] = 0.0
    return covs


def normalize(covs: torch.Tensor) -> torch.Tensor:
    return covs / torch.det(covs).unsqueeze(-1).unsqueeze(-1)


def apply_chain(covs: torch.Tensor, modifiers) -> torch.Tensor:
    for m in modifiers:
        covs = diagonalize(covs) if m == "diag" else normalize(covs)
    return covs
