"""Writes tests/golden/cov_models.npz: the reference's OWN observation-covariance classes (Module/Covariance/Project2to3.py:
GaussianMixtureCovariance, NoCovariance, Modifier_Diagonalize, Modifier_Normalize) run on CPU tensors.  Build-container only
(needs the reference checkout); imports it through tests.golden.make_golden.import_reference.

    python tests/golden/make_golden_cov_models.py
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.golden import make_golden as MG  # noqa: E402
from tools import synth  # noqa: E402

H, W, N = 120, 160, 48
CFG = dict(kernel_size=31, match_cov_default=0.25, min_flow_cov=0.25, min_depth_cov=0.05)


def inputs():
    """The covariance.npz inputs (same generators and seeds) plus rows that stress the mixture: very broad match covariances (weights
    near the 1e-3 threshold: near-uniform 1/961 ~ 1.04e-3 over the patch).  No NaN input row: the reference's batched pinverse raises on a
    non-finite covariance, so NaN propagation is checked on the GPU side against the finite rows (tests/test_gpu_cov_models.py)."""
    depth, dcov = synth.depth_maps(H, W, 3)
    kp = synth.keypoints(N, H, W, 5, border=20)
    g = torch.Generator().manual_seed(8)
    kpf = kp.float() + torch.rand(N, 2, generator=g)
    fcov = torch.exp(2 * 0.5 * torch.randn(N, 3, generator=g))
    fcov[:, 2] = 0.2 * torch.randn(N, generator=g) * fcov[:, :2].min(dim=1).values
    fcov[:4, 0] = 0.01
    fcov[:4, 2] = 0.0
    fcov[40:46, 0] = torch.tensor([1e3, 1e4, 1e5, 1e6, 3e2, 5e3])
    fcov[40:46, 1] = torch.tensor([1e3, 1e4, 1e5, 1e6, 2e3, 5e3])
    fcov[40:46, 2] = 0.0
    return depth, dcov, kp, kpf, fcov


def main():
    ref = MG.import_reference()
    P23 = ref.P23
    depth, dcov, kp, kpf, fcov = inputs()
    frame = SimpleNamespace(fx=160.0, fy=150.0, cx=80.0, cy=60.0)
    dest = SimpleNamespace(depth=depth, cov=dcov)
    gmm = P23.GaussianMixtureCovariance(SimpleNamespace(**CFG))
    out = {"depth": depth, "dcov": dcov, "kp_int": kp, "kp_float": kpf, "flow_cov_in": fcov.clone(),
           "K": np.array([frame.fx, frame.fy, frame.cx, frame.cy])}
    dc = dcov[0, 0, kp[:, 1], kp[:, 0]].contiguous()
    s0 = torch.ones(N, 3) * 0.25
    s0[:, 2] = 0
    out["depth_cov_kp"] = dc
    fc1 = fcov.clone()
    out["gmm_int_flowcov"] = gmm.estimate(frame, kp, dest, None, fc1)
    out["gmm_flow_cov_after"] = fc1
    out["gmm_float_flowcov"] = gmm.estimate(frame, kpf, dest, None, fcov.clone())
    out["gmm_int_nodefault"] = gmm.estimate(frame, kp, dest, dc, None)
    out["gmm_int_default_sigma"] = gmm.estimate(frame, kp, dest, dc, s0.clone())
    # the normalised Gaussian weights of the clamped covariances BEFORE the 1e-3 threshold (gaussain_full_kernels, patch-transposed
    # order = the order the weights meet the patch taps): where the threshold decisions fall
    cm = P23.create_2x2_matrix([[fc1[:, 0], fc1[:, 2]], [fc1[:, 2], fc1[:, 1]]], N, torch.device("cpu"))
    out["gmm_weights"] = ref.UM.gaussain_full_kernels(cm, 31).flatten(1)
    fcn = fcov.clone()
    out["none"] = P23.NoCovariance(None).estimate(frame, kpf, dest, None, fcn)
    out["none_flow_cov_after"] = fcn

    def nest(*types_, base="MatchCovariance"):
        cfg = SimpleNamespace(type=base, args=SimpleNamespace(**CFG, **({"device": "cpu"} if base == "MatchCovariance" else {})))
        for t in types_:
            cfg = SimpleNamespace(type=t, args=cfg)
        return P23.ICovariance2to3.instantiate(cfg.type, cfg.args)

    for key, chain, base in (("diag_match", ("Modifier_Diagonalize",), "MatchCovariance"),
                             ("norm_match", ("Modifier_Normalize",), "MatchCovariance"),
                             ("norm_diag_match", ("Modifier_Diagonalize", "Modifier_Normalize"), "MatchCovariance"),
                             ("diag_norm_match", ("Modifier_Normalize", "Modifier_Diagonalize"), "MatchCovariance"),
                             ("diag_gmm", ("Modifier_Diagonalize",), "GaussianMixtureCovariance")):
        m = nest(*chain, base=base)
        out[key] = m.estimate(frame, kpf, dest, None, fcov.clone())
    out["match_float_flowcov"] = P23.MatchCovariance(SimpleNamespace(**CFG, device="cpu")).estimate(frame, kpf, dest, None, fcov.clone())
    MG.save("cov_models", **out)


if __name__ == "__main__":
    main()
