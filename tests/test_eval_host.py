"""CPU: tests/eval_ref.py (the closed form the evaluation kernels implement) against the reference's own evaluate_flow / evaluate_flowcov /
evaluate_depth / evaluate_depthcov (tests/golden/eval.npz, written by tests/golden/make_golden_eval.py), the quantile and pinverse rules against
torch, the sequence reducers, and the new C-ABI symbols."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import eval_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLL = ("masked_nll", "q25_nll", "q50_nll", "q75_nll")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval.npz"))
    t = {k: torch.from_numpy(g[k]) for k in ("gt_flow", "est_flow", "flow_cov", "match_mask", "flow_mask", "gt_depth", "est_depth", "depth_cov")}
    return g, t


def golden_flow_frames(g, t, gtmask: bool, with_cov: bool, grids=None, sqrt="ieee"):
    """eval_ref over the golden's flow pairs with the reference's mask rules (EvalFlow.py:32-40, 86-92, 104-105)."""
    _, _, T, max_flow, _ = g["meta"]
    out = []
    for i in range(int(T) - 1):
        if gtmask:
            valid = t["flow_mask"][i, 0] & t["match_mask"][i, 0] if with_cov else t["flow_mask"][i, 0]
        else:
            valid = t["match_mask"][i, 0]
        out.append(ER.flow_frame(t["est_flow"][i], t["gt_flow"][i], t["flow_cov"][i] if with_cov else None, valid, float(max_flow), not gtmask, grids, sqrt))
    return out


@pytest.mark.parametrize("gtmask", [False, True])
def test_eval_ref_flow_matches_reference(golden, gtmask):
    g, t = golden
    tag = "_gtmask" if gtmask else ""
    # the records were made by torch on the CPU, whose fp32 sqrt is not the correctly rounded one the device has (eval_ref._sqrt): with that
    # sqrt the error fields are exact; with the IEEE one the rates stay exact and the means move by less than an ulp
    fr = golden_flow_frames(g, t, gtmask, False, sqrt="torch")
    ieee = golden_flow_frames(g, t, gtmask, False)
    for i, k in enumerate(("masked_epe_f32", "epe_f32", "px1", "px3", "px5")):          # error fields: exact
        assert abs(ER.seq_mean([f[k] for f in ieee]) - g["flow" + tag][i]) <= np.spacing(np.float32(g["flow" + tag][i])), k
        assert ER.seq_mean([f[k] for f in fr]) == g["flow" + tag][i], k
    grids = np.zeros((2, 100, 100), np.uint32)
    fr = golden_flow_frames(g, t, gtmask, True, grids)
    assert np.array_equal(grids, g["flowcov_grids" + tag])
    assert grids.sum() > 1000
    for i, k in enumerate(NLL):                                                         # within 4 x the closed form's distance from the SVD route
        assert abs(ER.seq_mean([f[k + "_f32"] for f in fr]) - g["flowcov" + tag][i]) <= 4 * g["flowcov_dist" + tag][i], k
        # ... and the fp64 mean of the same terms (what the kernels are compared with) within fp32 summation error of the reference's fp32 nanmean
        mean_abs = max(float(f["nll_px"][~torch.isnan(f["nll_px"])].abs().mean()) for f in fr)
        assert abs(ER.seq_mean([f[k] for f in fr]) - g["flowcov" + tag][i]) <= 4 * g["flowcov_dist" + tag][i] + 16 * 2.0 ** -24 * mean_abs, k


def test_eval_ref_depth_matches_reference(golden):
    g, t = golden
    _, _, T, _, max_depth = g["meta"]
    grid = np.zeros((100, 100), np.uint32)
    fr = [ER.depth_frame(t["est_depth"][i, 0], t["gt_depth"][i, 0], t["depth_cov"][i, 0], float(max_depth), grid) for i in range(int(T))]
    for i, k in enumerate(("masked_err_f32", "err_25", "err_50", "err_75")):            # (no sqrt in the depth error: exact either way)
        assert ER.seq_median([f[k] for f in fr]) == g["depth"][i], k
    assert np.array_equal(grid, g["depthcov_grid"]) and grid.sum() > 1000
    for i, k in enumerate(NLL):
        assert abs(ER.seq_mean([f[k + "_f32"] for f in fr]) - g["depthcov"][i]) <= 4 * g["depthcov_dist"][i], k


def _same(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_quantile_rule_is_torch_nanquantile():
    g = torch.Generator().manual_seed(3)
    inf = float("inf")
    cases = [torch.randn(n, generator=g) for n in (1, 2, 3, 4, 5, 9, 25, 101, 1000, 1961)]
    cases += [torch.exp(torch.randn(777, generator=g) * 8)]                                          # wide dynamic range
    cases += [torch.tensor([1.0, 2.0, inf, inf]), torch.tensor([inf, inf, inf]), torch.tensor([-inf, 0.0, 1.0, inf, inf, inf, inf, inf])]
    cases += [torch.full((17,), float("nan"))]
    cases += [torch.randint(0, 8, (403,), generator=g).float() * 0.37]                               # ties
    x = torch.randn(333, generator=g)
    x[::7] = float("nan")
    cases += [x]
    for v in cases:
        for q in (0.25, 0.5, 0.75):
            assert _same(ER.quantile(v, q), float(v.nanquantile(q))), (v.numel(), q)
        if not torch.isnan(v).all():
            assert _same(ER.lower_median(v), float(v.nanmedian())), v.numel()
    assert math.isnan(ER.quantile(torch.empty(0), 0.5)) and math.isnan(ER.lower_median(torch.empty(0)))


def test_pinv_rule_is_torch_pinverse():
    rows = torch.tensor([[1e-20, 1.0], [2.0, 0.0], [0.0, 0.0], [3.0, 5.0], [-2.0, 4.0], [1e-10, 1e6], [1e-9, 1e6], [-1e-20, -1.0], [0.5, 1e-30]])
    pu, pv = ER.pinv_diag2(rows[:, 0].clone(), rows[:, 1].clone())
    ref = torch.stack([torch.diag(r).pinverse().diagonal() for r in rows])
    assert torch.equal(torch.stack([pu, pv], 1), ref)
    assert (pu[0], pv[0]) == (0.0, 1.0) and (pu[1], pv[1]) == (0.5, 0.0)
    c = torch.tensor([0.0, 2.0, -4.0, 1e-30])
    assert torch.equal(ER.pinv_1(c), torch.stack([x.reshape(1, 1).pinverse().reshape(()) for x in c]))
    # det of the diagonal 2 x 2 is the product
    assert torch.equal(torch.stack([torch.diag(r).det() for r in rows[3:6]]), rows[3:6, 0] * rows[3:6, 1])


def test_sequence_reducers():
    from macvo_amd import evaluation as E

    vals = [E.DepthPerformance(4.0, 1.0, 2.0, 9.0), E.DepthPerformance(1.0, 3.0, 8.0, 3.0), E.DepthPerformance(3.0, 2.0, 4.0, 1.0),
            E.DepthPerformance(2.0, 7.0, 6.0, 5.0)]
    assert E.DepthPerformance.median(vals) == E.DepthPerformance(2.5, 2.5, 5.0, 4.0)        # even count: mean of the two middle values, per field
    assert E.DepthPerformance.median(vals[:3]) == E.DepthPerformance(3.0, 2.0, 4.0, 3.0)
    assert E.FlowPerformance.mean([E.FlowPerformance(1, 2, 3, 4, 5), E.FlowPerformance(3, 4, 5, 6, 7)]) == E.FlowPerformance(2, 3, 4, 5, 6)
    assert E.FlowCovPerformance.mean([E.FlowCovPerformance(1, 2, 3, 4), E.FlowCovPerformance(2, 4, 6, 8)]) == E.FlowCovPerformance(1.5, 3, 4.5, 6)
    with pytest.raises(ValueError):
        E.DepthCovPerformance.mean([])
    # a frame with an empty mask is skipped with a warning (EvalDepth.py:28-37)
    recs = [dict(masked_err=1.0, err_25=1.0, err_50=1.0, err_75=1.0, n_mask=5.0), dict(masked_err=float("nan"), err_25=float("nan"), err_50=float("nan"),
            err_75=float("nan"), n_mask=0.0), dict(masked_err=3.0, err_25=5.0, err_50=7.0, err_75=9.0, n_mask=2.0)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert E.depth_performance(recs, [10, 11, 12], 80.0) == E.DepthPerformance(2.0, 3.0, 4.0, 5.0)
    assert len(w) == 1 and "frame 11" in str(w[0].message)
    assert ER.seq_median([3.0, 1.0, 2.0, 10.0]) == 2.5


def test_eval_symbols_declared_and_bound():
    import macvo_amd._lib as L

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "macvo_hip.h")).read(), flags=re.S)
    for name in ("mv_eval_workspace_bytes", "mv_eval_flow_lanes", "mv_eval_depth_lanes"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    flow = re.search(r"enum\s*\{\s*(MV_EVAL_FLOW_MASKED_EPE.*?)\}", src, re.S).group(1)
    depth = re.search(r"enum\s*\{\s*(MV_EVAL_DEPTH_MASKED_ERR.*?)\}", src, re.S).group(1)
    names = [x.split("=")[0].strip() for x in flow.split(",")]
    assert [n[len("MV_EVAL_FLOW_"):].lower() for n in names] == list(L.EVAL_FLOW_COLS) + ["cols"]
    names = [x.split("=")[0].strip() for x in depth.split(",")]
    assert [n[len("MV_EVAL_DEPTH_"):].lower() for n in names] == list(L.EVAL_DEPTH_COLS) + ["cols"]
    assert L.ABI_VERSION == 8
    lib = L.load()
    assert lib.mv_abi_version() == 8
    assert lib.mv_eval_workspace_bytes(1, 480, 640) > 0 and lib.mv_eval_workspace_bytes(1, 2048, 2048) > 0
    assert lib.mv_eval_workspace_bytes(1, 2048, 2049) == 0 and lib.mv_eval_workspace_bytes(65, 4, 4) == 0
    assert lib.mv_eval_workspace_bytes(2, 480, 640) > lib.mv_eval_workspace_bytes(1, 480, 640)
