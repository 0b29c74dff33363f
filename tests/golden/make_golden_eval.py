"""Writes tests/golden/eval.npz: the reference's OWN evaluate_flow / evaluate_flowcov (Evaluation/EvalFlow.py) and evaluate_depth /
evaluate_depthcov (Evaluation/EvalDepth.py), imported in place through tests.golden.make_golden.import_reference (the module finder stubs what is
missing) and driven with a fake matcher / depth module and a plain list of frames.  Plotting is stubbed (plot_flow_performance,
GridRecorder.plot_figure); the recorders' grids are captured.  All four functions import and run under the stubs.  Build-container only.

    python tests/golden/make_golden_eval.py

Also stored: for every NLL field, the largest per-pixel distance, within that field's population, between tests/eval_ref.py's fp32 closed form and
the reference's route (batched det().log() + MahalanobisDist(...).square(), i.e. SVD pinverse + bmm) on the same inputs — the scale of the
tolerance tests/test_eval_host.py allows on the NLL means."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import eval_ref as ER  # noqa: E402
from tests.golden import make_golden as MG  # noqa: E402

H, W, T = 37, 53, 3
MAX_FLOW, MAX_DEPTH = 6.0, 30.0


def inputs():
    """Three frames: estimates = ground truth + seeded error, covariances exp(N), 3 % NaN ground truth, a matcher mask, a ground-truth flow mask."""
    g = torch.Generator().manual_seed(77)
    o = {}
    o["gt_flow"] = torch.randn(T, 2, H, W, generator=g) * 4
    o["est_flow"] = o["gt_flow"][:T - 1] + torch.randn(T - 1, 2, H, W, generator=g) * torch.exp(torch.randn(T - 1, 2, H, W, generator=g))
    o["flow_cov"] = torch.cat([torch.exp(torch.randn(T - 1, 2, H, W, generator=g) * 1.5), torch.zeros(T - 1, 1, H, W)], 1)
    o["match_mask"] = torch.rand(T - 1, 1, H, W, generator=g) > 0.1
    o["flow_mask"] = torch.rand(T, 1, H, W, generator=g) > 0.2
    o["gt_depth"] = torch.rand(T, 1, H, W, generator=g) * 40 + 0.5
    o["est_depth"] = o["gt_depth"] + torch.randn(T, 1, H, W, generator=g) * torch.exp(torch.randn(T, 1, H, W, generator=g))
    o["depth_cov"] = torch.exp(torch.randn(T, 1, H, W, generator=g) * 1.5)
    o["gt_flow"][torch.rand(T, 2, H, W, generator=g) < 0.03] = float("nan")
    o["gt_depth"][torch.rand(T, 1, H, W, generator=g) < 0.03] = float("nan")
    return o


def frames_of(o):
    return [SimpleNamespace(frame_idx=t, stereo=SimpleNamespace(idx=t, gt_flow=o["gt_flow"][t:t + 1].clone(), flow_mask=o["flow_mask"][t:t + 1].clone(),
                                                               gt_depth=o["gt_depth"][t:t + 1].clone())) for t in range(T)]


class FakeMatcher:
    provide_cov = True

    def __init__(self, o):
        self.o = o

    def estimate(self, a, b):
        t = a.idx
        return SimpleNamespace(flow=self.o["est_flow"][t:t + 1].clone(), cov=self.o["flow_cov"][t:t + 1].clone(), mask=self.o["match_mask"][t:t + 1].clone())


class FakeDepth:
    provide_cov = True

    def __init__(self, o):
        self.o = o

    def estimate(self, a):
        t = a.idx
        return SimpleNamespace(depth=self.o["est_depth"][t:t + 1].clone(), cov=self.o["depth_cov"][t:t + 1].clone(), mask=None)


def main():
    ref = MG.import_reference()
    import Evaluation.EvalDepth as ED
    import Evaluation.EvalFlow as EF
    from Utility.Extensions import GridRecorder

    made = []

    class Recorder(GridRecorder):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

        def plot_figure(self, *a, **k):
            return SimpleNamespace(savefig=lambda *a, **k: None)

    EF.GridRecorder = ED.GridRecorder = Recorder
    EF.plot_flow_performance = lambda *a, **k: None
    o = inputs()
    out = dict(o)
    out["meta"] = np.array([H, W, T, MAX_FLOW, MAX_DEPTH], dtype=np.float64)

    def rec(r):
        return np.array(list(vars(r).values()), dtype=np.float64)

    for tag, gtm in (("", False), ("_gtmask", True)):
        out["flow" + tag] = rec(EF.evaluate_flow(FakeMatcher(o), frames_of(o), MAX_FLOW, None, gtm))
        made.clear()
        out["flowcov" + tag] = rec(EF.evaluate_flowcov(FakeMatcher(o), frames_of(o), MAX_FLOW, gtm))
        out["flowcov_grids" + tag] = np.stack([made[0].grid, made[1].grid])
    out["depth"] = rec(ED.evaluate_depth(FakeDepth(o), frames_of(o), MAX_DEPTH))
    made.clear()
    out["depthcov"] = rec(ED.evaluate_depthcov(FakeDepth(o), frames_of(o), MAX_DEPTH))
    out["depthcov_grid"] = made[0].grid

    # per-pixel distance of the closed form from the reference's route, per NLL field's population (worst frame)
    def worst(d, pop):
        d = d[pop & ~torch.isnan(d)]
        return float(d.max()) if d.numel() else 0.0

    fd, dd = np.zeros((2, 4)), np.zeros(4)
    for t in range(T - 1):
        est, gt, cov = o["est_flow"][t], o["gt_flow"][t], o["flow_cov"][t, :2]
        cm = cov.permute(1, 2, 0).diag_embed().flatten(end_dim=1)
        em = (est - gt).permute(1, 2, 0).flatten(end_dim=1)
        svd = (cm.det().log().view(-1, 1, 1) + ref.UM.MahalanobisDist(em, torch.zeros_like(em), cm).square()).reshape(H, W)
        for gi, gtm in enumerate((False, True)):
            valid = (o["flow_mask"][t, 0] & o["match_mask"][t, 0]) if gtm else o["match_mask"][t, 0]
            fr = ER.flow_frame(est, gt, cov, valid, MAX_FLOW, apply_max_flow=not gtm)
            d = (fr["nll_px"] - svd).abs()
            pops = [fr["mask_px"]] + [fr["unc_px"] < fr[f"t{q}"] for q in ("25", "50", "75")]
            fd[gi] = np.maximum(fd[gi], [worst(d, p) for p in pops])
    for t in range(T):
        est, gt, cov = o["est_depth"][t, 0], o["gt_depth"][t, 0], o["depth_cov"][t, 0]
        cm = cov.reshape(-1, 1, 1)
        em = (est - gt).reshape(-1, 1)
        svd = (cm.det().log().view(-1, 1, 1) + ref.UM.MahalanobisDist(em, torch.zeros_like(em), cm).square()).reshape(H, W)
        fr = ER.depth_frame(est, gt, cov, MAX_DEPTH)
        d = (fr["nll_px"] - svd).abs()
        pops = [fr["mask_px"]] + [fr["unc_px"] < fr[f"t{q}"] for q in ("25", "50", "75")]
        dd = np.maximum(dd, [worst(d, p) for p in pops])
    out["flowcov_dist"], out["flowcov_dist_gtmask"], out["depthcov_dist"] = fd[0], fd[1], dd
    print("per-pixel |closed form - SVD route| per NLL field: flow", fd, "depth", dd)
    MG.save("eval", **out)


if __name__ == "__main__":
    main()
